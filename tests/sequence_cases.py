"""The step table of the context sequence tests: every family of operation of the engine as one step,
built and answered on the CPU. TEST INFRASTRUCTURE ONLY.

A step is a name, an operation, its host inputs (from a seed derived from the name, with the suite's own
generators) and either the expected result, computed once by the CPU side the suite trusts (the oracle and
the Python models on top of it), or the name of an earlier step (src) whose DEVICE output it consumes in
place: a ct_mul output is a capacity-padded CSR batch, and its consumer's expectation is the model applied
to the producer's model output. Each step also declares its route: the delta of every counter of the
engine (counters() in test_gpu_sequence.py); a counter it does not name must not move. The general ct_mul
path's iblk and direct counts come from large_route(), a restatement of build_large_desc and
assign_static_groups (large_plan.hpp, rt_mul.cpp); a gather's tiles from gather_tiles.hpp's geometry.

Two parameter sets. A context cannot change its edge_budget, and a 64-lane ct_add pair with a tail loop
needs more than 3 * 64 = 192 edges, so the steps run as
  main: B = 337, m_bits = 8192, the fixture key's canon_tag, edge_budget = 120 (test_merge_vs_oracle's:
        pairs under and over the budget mix). Every step but seven.
  wide: the same at edge_budget = 1,200,000: the 33- and 64-layer ct_add / ct_sub steps
        (k_ct_add_wave<64>), a ct_mul above 120 edges that stays in hash order, its output added, and
        test_direct_cancelling_key_redo_vs_oracle's batch on the general path's direct mode (at 120 every
        direct pair is over the budget and redone).
Each set is one sequence on one context (test_gpu_sequence.py); test_sequence_cases.py checks on the CPU
that every step is the case it claims to be."""
import os
import zlib

import numpy as np

import gather_model as gam
import gsum_model as gm
import lincomb_model as lm
import recrypt_model as rm
from helpers import (LAYER_DT, REF, Cipher, fixture_secret, pack_meta, read_ct, read_u64, splitmix_stream, sumdigest,
                     write_ct)
from test_gpu_add_merge import _mk as mk_add
from test_gpu_compact_layers import family
from test_gpu_large import _mk as mk_mul
from test_gpu_large import _mk_layers as mk_layers
from test_gpu_recrypt import _plain, _skew, _uniform_sigma

B = 337
M_BITS = 8192
BUDGET = {"main": 120, "wide": 1200000}
LIMIT_DEFAULT, LIMIT_DEEP = 16384, 1 << 16
P = (1 << 127) - 1
M64 = (1 << 64) - 1
EINVAL, ENOSYS = -22, -38
PRE = 3   # k_ct.hip kPre: edges a lane of k_ct_add_wave holds in registers; the tail loops start at PRE * G

# the table's order; test_sequence_cases.py holds build() to it
STEP_NAMES = {
    "main": ["mul_fresh", "check_gsum", "mul_cancel", "mul_general", "mul_sigma", "mul_over", "mul_pending",
             "add32", "sub32", "add65", "sub65", "add_deep", "add_many", "merge_add", "merge_sub",
             "sum_routes", "sum_fold", "sum_deep", "compact_routes", "recrypt",
             "commit", "image", "gather", "metrics", "dec", "enc", "scale", "neg", "chain",
             "link_add", "link_sum", "link_compact", "link_dec", "link_scale", "link_commit_image",
             "ref_stale", "ref_sizes", "ref_layer_limit", "ref_lincomb_status", "ref_mul_status"],
    "wide": ["add33", "sub33", "add64", "sub64", "mul_wide", "link_add_wide", "mul_direct"],
}
# operations that read or write none of the plan scratch and take no plan stamp (rt_*.cpp: no plan_pass,
# no ps.invalidate(); a chain runs its plans on worker contexts): a pending ct_mul plan stays valid across
# them. mul_pending runs exactly these, in this order, between ct_mul_plan and ct_mul(plan=...):
# test_gpu_sequence.py keeps one call per name and runs the list.
PENDING_SAFE = ["dec_value", "gather_select", "gather_cat", "ct_scale", "commit_ct", "ct_image", "ct_from_image",
                "sigma_bytehist", "layer_gsum", "sigma_popcount", "ubk_apply", "digest", "sumdigest", "pack",
                "fp_binop", "fp_inv", "fill_random", "drbg_fill", "drbg_reseed", "aes256_ctr", "prf", "enc_value",
                "enc_value_depth", "enc_items", "base_R", "sigma", "gen_fresh", "fill_nonces", "check_mul_gsum",
                "ct_mul_chain", "set_layer_limit", "timing_reset"]


class Step:
    def __init__(self, name, op, pset="main", src=None, limit=LIMIT_DEFAULT, **inp):
        self.name, self.op, self.pset, self.src, self.limit = name, op, pset, src, limit
        self.inp = inp        # host inputs
        self.want = {}        # expected values, compared exactly
        self.route = {}       # counter deltas; every other counter stays put
        self.refuse = None    # (status code, message part) of a step the host refuses
        self.out = None       # the model's output ciphers: what a consumer's model reads
        self.aux = {}         # what the CPU test or a consumer needs besides
        self.size = 0         # input rows: orders "large then small"


def seed_of(name):
    return zlib.crc32(name.encode())


def keys():
    """The key material every step shares, set once on a context."""
    sk, man, em = fixture_secret()
    return {"canon_tag": man["canon_tag"], "H_digest": bytes.fromhex(man["H_digest"]), "powg": read_u64("powg_B.u64"),
            "prf_k": read_u64("sk_prf_k.u64"), "lpn_s": read_u64("sk_lpn_s.u64"), "em": em, "sk": sk,
            "ubk_inv": rm.gen_ubk(man["canon_tag"], M_BITS)[1]}


# ---------------------------------------------------------------------------------------- generators
def closure_cipher(rng, n, ne, tail=False, twin_of=None):
    """n >= 9 layers for the ct_add wave kernels' closure: a PROD chain three deep from the LAST layer,
    n-1 -> 2 -> n-2 -> 4, so the parent n-2 lies above its child 2, the BASE layers 4 (end of the chain), 0
    and 1 are parents, and no edge names 1, 2, 4 or n-2: group_close needs three rounds and an ascending
    sweep does not close the set. Edges sit on layers 0, 5 and n-1; every other layer is dropped. tail: the
    cipher's LAST edge is the only one on layer 7. twin_of: the same layers with an edge on every one (the
    identity remap)."""
    if twin_of is None:
        lay = np.zeros(n, LAYER_DT)
        for f in ("ztag", "nonce_lo", "nonce_hi"):
            lay[f] = rng.integers(0, 2**63, n, dtype=np.uint64)
        lay[n - 1] = (1, 2, 0, 0, 0, 0, 0)
        lay[2] = (1, n - 2, 1, 0, 0, 0, 0)
        lay[n - 2] = (1, 4, 4, 0, 0, 0, 0)
        on = [0, 5, n - 1]
    else:
        lay, on = twin_of.layers.copy(), list(range(n))
    lid = np.asarray(on, np.uint64)[rng.integers(0, len(on), ne)]
    lid[:len(on)] = on
    rng.shuffle(lid)
    if tail:
        lid[-1] = 7
        assert all(l in lid[:-1] for l in on if l != 7)
    meta = pack_meta(lid, rng.integers(0, B, ne), rng.integers(0, 2, ne))
    return Cipher(lay, meta, rng.integers(0, 2**64, ne, dtype=np.uint64), rng.integers(0, 2**63, ne, dtype=np.uint64),
                  rng.integers(0, 2**64, (ne, 128), dtype=np.uint64))


def closure_pairs(rng, L, G):
    """Three pairs (odd: the last lane group of the last wave has none) of L layers and more than PRE * G
    edges each: a closure pair, its identity twin, a second closure pair. The tail-only layer is B's layer 7,
    named by the last edge of the concatenation."""
    la, lb = L - L // 2, L // 2
    na, nb = (50, 60) if G == 32 else (100, 110)
    assert na + nb > PRE * G
    xs, ys = [], []
    for k in range(2):
        x, y = closure_cipher(rng, la, na), closure_cipher(rng, lb, nb, tail=True)
        xs.append(x); ys.append(y)
        if k == 0:
            xs.append(closure_cipher(rng, la, na, twin_of=x)); ys.append(closure_cipher(rng, lb, nb, twin_of=y))
    return xs, ys


def is_fresh_pair(orc, x, y):
    """k_plan_mul's class of a pair (k_ct.hip): the fresh kernel or the general path."""
    keys_, prod, cap_l = x.nL * y.nL * B, x.nE * y.nE, x.nL + y.nL + x.nL * y.nL
    return (keys_ <= 1536 and prod <= 4096 and x.nE <= 256 and y.nE <= 256 and cap_l <= 64 and
            orc.bucket_count(prod) + prod + 3 <= 3 * keys_)


def narrow_pair(rng, na=40, nb=40):
    """A fresh-shape pair (2 x 2 layers) the fresh kernel finishes itself at edge_budget 120: enough products
    (na * nb) for a bucket count that keeps its key slots apart, on idx ranges of 8 and 7, so the products
    fall into at most 4 * 14 * 2 = 112 cells."""
    return lm.strip(mk_add(rng, 2, na, idx_range=8)), lm.strip(mk_add(rng, 2, nb, idx_range=7))


def cancelling_pair(rng):
    """test_direct_cancelling_key_redo_vs_oracle's construction at the fresh shape: the first A weight is
    solved so that the P cell its product with a B edge of its channel falls into sums to 0 mod p. The cell's
    edge is dropped (arithmetic.hpp:96-101), which the fresh kernel leaves to the general path."""
    x, y = narrow_pair(rng)
    w = lambda c, k: (int(c.w_lo[k]) | (int(c.w_hi[k]) << 64)) % P
    j0 = int(np.flatnonzero(y.ch() == x.ch()[0])[0])
    r = (int(x.idx()[0]) + int(y.idx()[j0])) % B
    terms = [(k, j) for k in range(x.nE) for j in range(y.nE)
             if x.layer_id()[k] == x.layer_id()[0] and y.layer_id()[j] == y.layer_id()[j0] and x.ch()[k] == y.ch()[j] and
             (int(x.idx()[k]) + int(y.idx()[j])) % B == r]
    assert (0, j0) in terms and len(terms) > 2
    coef = sum(w(y, j) for k, j in terms if k == 0) % P
    rest = sum(w(x, k) * w(y, j) for k, j in terms if k != 0) % P
    v = (-rest * pow(coef, P - 2, P)) % P
    assert coef != 0 and v != 0
    x.w_lo[0], x.w_hi[0] = np.uint64(v & M64), np.uint64(v >> 64)
    assert sum(w(x, k) * w(y, j) for k, j in terms) % P == 0
    return x, y


def cancel_direct(x, y, r=5):
    """The original construction: A's layer 0 holds every (idx, ch) cell once, and the A weight that meets B's
    first layer-0 edge in the P cell of key (0, 0, r) is solved so that the cell sums to 0 mod p."""
    w = lambda c, k: (int(c.w_lo[k]) | (int(c.w_hi[k]) << 64)) % P
    a_at = {(int(i), int(c)): k for k, (l, i, c) in enumerate(zip(x.layer_id(), x.idx(), x.ch())) if l == 0}
    terms = [(a_at[((r - int(y.idx()[j])) % B, int(y.ch()[j]))], j) for j in range(y.nE) if y.layer_id()[j] == 0]
    (k0, j0), rest = terms[0], terms[1:]
    v = (-sum(w(x, k) * w(y, j) for k, j in rest) * pow(w(y, j0), P - 2, P)) % P
    x.w_lo[k0], x.w_hi[k0] = np.uint64(v & M64), np.uint64(v >> 64)
    assert len(terms) == 20 and sum(w(x, k) * w(y, j) for k, j in terms) % P == 0


def product_cells(x, y):
    """Distinct (layer pair, idx, P / M) cells of a pair's products."""
    lay = x.layer_id().astype(np.int64)[:, None] * y.nL + y.layer_id().astype(np.int64)[None, :]
    idx = (x.idx().astype(np.int64)[:, None] + y.idx().astype(np.int64)[None, :]) % B
    pm = (x.ch()[:, None] != y.ch()[None, :]).astype(np.int64)
    return len(np.unique((lay * B + idx) * 2 + pm))


# ---------------------------------------------------------------------------------------- models
def slots_share_bucket(nb, S):
    """large_plan.hpp: whether two key slots of [0, S) share a libstdc++ bucket among nb."""
    if S > nb:
        return True
    keys_ = [(((s // B) << 32) | (s % B)) * 0x9E3779B97F4A7C15 % (1 << 64) % nb for s in range(S)]
    return len(set(keys_)) < S


def large_route(orc, x, y, budget, allow_direct=True):
    """(iblk, direct) of a general-path pair: build_large_desc after assign_static_groups. A pair whose bucket
    count is at least twice its key slots takes the static groups and, with at most 4 B layers and 63 B edges,
    the iblk order; of those a pair whose slots share no bucket runs the direct mode (B = 337 and <= 4 staged B
    layers fit its LDS: test_direct_mode_shapes_vs_oracle runs them at B = 1,024)."""
    S, n = x.nL * y.nL * B, x.nE * y.nE
    nb = orc.bucket_count(n)
    assert x.nL + y.nL + x.nL * y.nL <= 16384 and y.nL <= 4
    static = S > 0 and nb >= 2 * S
    iblk = static and y.nL <= 4 and x.nE >= 1 and 1 <= y.nE <= 63
    direct = iblk and allow_direct and budget < 1 << 28 and x.nE < 1 << 21 and not slots_share_bucket(nb, S)
    return int(iblk), int(direct)


def gather_tiles(ciphers, sigma_words=128):
    """gather_tiles.hpp: tiles of one gather exec over its output ciphers (16 KiB of edge rows or layers each)."""
    ept, lpt = max(16384 // (24 + 8 * sigma_words), 1), 16384 // 40
    return sum(-(-c.nE // ept) - (-c.nL // lpt) for c in ciphers)


def mul_layout(xs, ys):
    """ct_mul_plan's capacities (k_plan_mul): exclusive scans of the layer and edge slots, and the totals."""
    cap_l = [x.nL + y.nL + x.nL * y.nL for x, y in zip(xs, ys)]
    cap_e = [2 * min(x.nE * y.nE, x.nL * y.nL * B) for x, y in zip(xs, ys)]
    l_off = np.concatenate([[0], np.cumsum(cap_l)[:-1]]).astype(np.int64)
    e_off = np.concatenate([[0], np.cumsum(cap_e)[:-1]]).astype(np.int64)
    return l_off, e_off, int(sum(cap_l)), int(sum(cap_e))


def mul_model(ctx, st, xs, ys, seed, sigma=False, redo=()):
    """Fills a ct_mul step: nonces (and salts) over the planned slots, the oracle's product of every pair,
    the plan's classes and the route. redo: the pairs the fresh kernel or the direct mode flags, which the
    general path runs again on its full layout (no direct mode there)."""
    orc, budget = ctx["oracle"], BUDGET[st.pset]
    l_off, e_off, tl, te = mul_layout(xs, ys)
    rng = np.random.default_rng(seed)
    nonces = rng.integers(0, 2**63, 2 * max(tl, 1), dtype=np.uint64)
    salts = rng.integers(0, 2**63, max(te, 1), dtype=np.uint64) if sigma else None
    out, per = [], []
    for p, (x, y) in enumerate(zip(xs, ys)):
        base = int(l_off[p]) + x.nL + y.nL
        nz = nonces[2 * base:2 * base + 2 * x.nL * y.nL].copy()
        per.append(nz)
        out.append(orc.ct_mul(lm.strip(x), lm.strip(y), nz, salts=None if salts is None else salts[int(e_off[p]):],
                              H=ctx["H"]() if sigma else None, canon_tag=ctx["keys"]["canon_tag"], edge_budget=budget))
    small = [is_fresh_pair(orc, x, y) for x, y in zip(xs, ys)]
    n_small = sum(small)
    routes = [large_route(orc, x, y, budget) for x, y, s in zip(xs, ys, small) if not s]
    routes += [large_route(orc, xs[p], ys[p], budget, allow_direct=False) for p in redo]
    st.inp.update(xs=xs, ys=ys, nonces=nonces, salts=salts, sigma=sigma)
    st.out = out
    st.aux.update(l_off=l_off, e_off=e_off, per=per)
    st.want.update(out=out, n_small=n_small, n_large=len(xs) - n_small, layer_slots=tl, edge_slots=te)
    st.route = {"mul.fresh": n_small, "mul.general": len(routes), "mul.redo": len(redo),
                "mul.iblk": sum(r[0] for r in routes), "mul.direct": sum(r[1] for r in routes)}
    st.size = sum(c.nE + c.nL for c in xs + ys)


def add_model(ctx, st, xs, ys, negate, sigma):
    orc, budget = ctx["oracle"], BUDGET[st.pset]
    pick = (lambda c: c) if sigma else lm.strip
    out = [orc.ct_add(pick(x), pick(y), negate=negate, edge_budget=budget) for x, y in zip(xs, ys)]
    st.inp.update(negate=negate, sigma=sigma)
    st.out = out
    st.aux.update(xs=xs, ys=ys)
    max_layers = max(x.nL + y.nL for x, y in zip(xs, ys))
    st.want.update(out=out, n_large=sum(x.nE + y.nE > budget for x, y in zip(xs, ys)), max_layers=max_layers)
    st.route = {"deep.add": 1} if max_layers > 30000 else {}
    st.size = sum(c.nE + c.nL for c in xs + ys)


def lincomb_model(ctx, st, pool, segs, scales=None, flags=None, status=None):
    orc, budget = ctx["oracle"], BUDGET[st.pset]
    seg_off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint64)
    term = np.array([t for s in segs for t in s], np.uint64)
    out = lm.fold_segments(orc, pool, seg_off, term, scales, flags, edge_budget=budget)
    st.inp.update(seg_off=seg_off, term=term, scales=scales, flags=flags)
    st.out = out
    st.aux.update(pool=pool)
    # 0 one pass, 1 fold (over edge_budget), 2 fold (a term out of contract: given by the caller)
    over = [sum(pool[int(t)].nE for t in s) > budget for s in segs]
    st.want.update(out=out, status=[int(o) for o in over] if status is None else status)
    n_fold = sum(1 for s in st.want["status"] if s)
    deep = sum(pool[int(t)].nL > 30000 for t in term)
    wg = sum(64 < pool[int(t)].nL <= 30000 for t in term)
    st.route = {"lin.one_pass": len(segs) - n_fold, "lin.fold": n_fold, "lin.wave_terms": len(term) - wg - deep,
                "lin.wg_terms": wg, "deep.lin_terms": deep}
    st.size = sum(pool[int(t)].nE + pool[int(t)].nL for t in term)


def compact_class(c):
    """k_compact_plan's class (k_recrypt.hip): the batched kernel holds 14,336 cells."""
    return "small" if c.nE == 0 or c.nL == 0 or (c.nL <= 1024 and c.nE <= 1 << 16 and c.nL * 2 * B <= 14336) else "merge"


def recrypt_one(orc, x, pool, picks, inv, budget):
    """recrypt_model.recrypt with the context's edge_budget in the loop's ct_add; also the cipher the final
    compaction reads (None: returned as it came)."""
    if not pool or x.nE == 0:
        return x, 0, None
    res, it = x, 0
    while it < 8 and rm.needs_balance(rm.popcount(res.sigma), res.nE, M_BITS):
        res = orc.ct_add(res, pool[int(picks[it]) % len(pool)], edge_budget=budget)
        res = Cipher(res.layers, res.meta, res.w_lo, res.w_hi, rm.apply_perm(res.sigma, inv, M_BITS))
        it += 1
    return rm.compact(orc, res), it, res


def dec_model(ctx, st, cs, l_off, slots, seed):
    """dec_value of ciphers whose layers sit at l_off[i] of `slots` layer slots: a random R per slot (the
    BASE ones are read), the oracle's value per cipher."""
    R = np.random.default_rng(seed).integers(1, 2**63, 2 * max(slots, 1), dtype=np.uint64)
    vals = []
    for c, o in zip(cs, l_off):
        lo, hi = ctx["oracle"].dec(lm.strip(c), ctx["keys"]["powg"], R[2 * int(o):2 * (int(o) + c.nL)])
        vals.append(lo | (hi << 64))
    st.inp.update(R=R)
    st.want.update(values=vals, status=[0] * len(cs))


def dense_off(cs):
    return np.concatenate([[0], np.cumsum([c.nL for c in cs])[:-1]]).astype(np.int64) if cs else np.zeros(0, np.int64)


def file_view(c):
    """The cipher as the .ct format keeps it: a PROD layer's seeds and a BASE layer's parents are not stored."""
    L = c.layers.copy()
    prod = L["rule"] == 1
    for f in ("ztag", "nonce_lo", "nonce_hi"):
        L[f][prod] = 0
    L["pa"][~prod] = 0
    L["pb"][~prod] = 0
    return Cipher(L, c.meta, c.w_lo, c.w_hi, c.sigma)


def commit_image_model(ctx, st, cs, sigma):
    k = ctx["keys"]
    pick = (lambda c: c) if sigma else lm.strip
    st.inp.update(sigma=sigma)
    st.want.update(commit=[ctx["oracle"].commit(pick(c), k["canon_tag"], k["H_digest"]) for c in cs],
                   image=write_ct([pick(c) for c in cs], nbits=M_BITS), out=[file_view(pick(c)) for c in cs])
    st.aux.update(layer_cap=sum(c.nL for c in cs), edge_cap=sum(c.nE for c in cs))
    st.route = {"img.write_wide": 1, "img.parse_wide": 1} if sigma else {"img.write_narrow": 1, "img.parse_narrow": 1}


# ---------------------------------------------------------------------------------------- the table
def build(oracle):
    """Every step of both sets, inputs and expectations, in STEP_NAMES' order: {set: [Step]}."""
    H = {}

    def dense_H():
        if "H" not in H:
            H["H"], d = oracle.gen_H(ctx["keys"]["canon_tag"])
            assert d == ctx["keys"]["H_digest"]
        return H["H"]

    ctx = {"oracle": oracle, "keys": keys(), "H": dense_H}
    k = ctx["keys"]
    T = {"main": [], "wide": []}
    by = {}

    def step(name, op, **kw):
        st = Step(name, op, **kw)
        T[st.pset].append(st)
        by[name] = st
        return st, np.random.default_rng(seed_of(name))

    # a pair of few products has few buckets for its 1,348 key slots: the fresh kernel starts it and leaves it
    # to the general path (k_mul_fresh.hip, F3_BIGOVF), which counts as a redo
    tiny = lambda rng, na, nb: (mk_mul(rng, 2, na, dup_ok=False), mk_mul(rng, 2, nb, dup_ok=False))
    fresh = lambda rng, na, nb: narrow_pair(rng, na, nb)
    general = lambda rng: (mk_mul(rng, 8, 12, dup_ok=False), mk_mul(rng, 2, 8, dup_ok=False))
    split = lambda pairs: ([p[0] for p in pairs], [p[1] for p in pairs])

    # ---- ct_mul
    st, rng = step("mul_fresh", "mul")           # 5 fresh x fresh pairs, every product within the budget
    mul_model(ctx, st, *split([fresh(rng, 40 - p % 3, 40 - 2 * (p % 2)) for p in range(5)]), seed_of("mul_fresh") + 1)
    st.want["status"] = [0] * 5
    st, _ = step("check_gsum", "check_gsum", src="mul_fresh")
    src = by["mul_fresh"]
    st.want.update(bad=0, status=[gm.status(oracle, x, y, c, nz, k["powg"], B)
                                  for x, y, c, nz in zip(src.inp["xs"], src.inp["ys"], src.out, src.aux["per"])])
    st.route = {"gsum.lds": 1}
    st, rng = step("mul_cancel", "mul")          # fresh, general and the cancelling pair: one redo
    pairs = [fresh(rng, 40, 39), general(rng), cancelling_pair(rng), fresh(rng, 37, 40)]
    mul_model(ctx, st, *split(pairs), seed_of("mul_cancel") + 1, redo=[2])
    st.want["status"] = [0] * 4
    st.aux["cancel"] = 2
    st, rng = step("mul_general", "mul")         # two general-path pairs, 8 layers x 2 layers
    mul_model(ctx, st, *split([general(rng), general(rng)]), seed_of("mul_general") + 1)
    st.want["status"] = [0] * 2
    st, rng = step("mul_sigma", "mul")           # WITH_SIGMA over both paths
    mul_model(ctx, st, *split([fresh(rng, 40, 38), general(rng), fresh(rng, 36, 40)]), seed_of("mul_sigma") + 1, sigma=True)
    st.want["status"] = [0] * 3
    st, rng = step("mul_over", "mul")            # fresh shapes above the budget: canonical order, by the general path
    mul_model(ctx, st, *split([(lm.strip(mk_add(rng, 2, 40)), lm.strip(mk_add(rng, 2, 40 - q))) for q in range(3)]),
              seed_of("mul_over") + 1, redo=[0, 1, 2])
    st.want["status"] = [1] * 3
    st, rng = step("mul_pending", "mul_pending")  # ct_mul_plan, every PENDING_SAFE operation, ct_mul(plan=...)
    mul_model(ctx, st, *split([fresh(rng, 40, 40), general(rng), fresh(rng, 38, 39)]), seed_of("mul_pending") + 1)
    st.want["status"] = [0] * 3
    mid = [_plain(rng, 2, 30, M_BITS, first=i) for i in range(3)]
    st.inp.update(mid=mid, mid_R=rng.integers(1, 2**63, 2 * 6, dtype=np.uint64),
                  enc_vals=rng.integers(0, 2**64, 2, dtype=np.uint64), enc_rnd=rng.integers(0, 2**64, (2, 256), dtype=np.uint64))
    # what the operations in between count: select + cat (3 + 6 ciphers), bytehist, layer_gsum, image + parse,
    # enc_value of 2, enc_value_depth of 1 and enc_items of 2 (a sub-batch and a run each), check_mul_gsum
    st.route.update({"gather.wide": 2, "gather.ciphers": 9, "gather.tiles": 3 * gather_tiles(mid), "metrics.hist_wide": 1,
                     "metrics.gsum_wave": 3, "img.write_wide": 1, "img.parse_wide": 1, "enc.narrow": 5, "enc.sub": 3,
                     "enc.runs": 3, "gsum.lds": 1})

    # ---- ct_add / ct_sub under the budget, by kernel
    for name, L, G, pset in (("add32", 32, 32, "main"), ("sub32", 32, 32, "main"), ("add65", 65, 64, "main"),
                             ("sub65", 65, 64, "main"), ("add33", 33, 64, "wide"), ("sub33", 33, 64, "wide"),
                             ("add64", 64, 64, "wide"), ("sub64", 64, 64, "wide")):
        st, rng = step(name, "add", pset=pset)
        # 65 layers: k_ct_add, whose loops have no register part; the pairs keep their shape within the budget
        xs, ys = closure_pairs(rng, L, 32 if pset == "main" else G)
        add_model(ctx, st, xs, ys, name.startswith("sub"), True)
        st.inp.update(xs=xs, ys=ys)
        st.aux.update(L=L, G=G if L != 65 else 0, twins=[False, True, False])
    for name in ("add_deep",):                   # one pair of 30,001 layers: k_ct_add_deep
        st, rng = step(name, "add", limit=LIMIT_DEEP)
        xs, ys = [family(rng, 15001, sigma=True)], [family(rng, 15000, sigma=True)]
        add_model(ctx, st, xs, ys, False, True)
        st.inp.update(xs=xs, ys=ys)
        st.aux.update(L=30001, G=0, twins=[False])

    st, rng = step("add_many", "add")            # 1,025 pairs: one above the floor of the per-pair plan scratch, which regrows
    xs, ys = [lm.strip(mk_add(rng, 1, 1)) for _ in range(1025)], [lm.strip(mk_add(rng, 1, 1)) for _ in range(1025)]
    add_model(ctx, st, xs, ys, False, False)
    st.inp.update(xs=xs, ys=ys)

    # ---- ct_add / ct_sub over the budget: the merge route (test_merge_vs_oracle's kinds)
    for name in ("merge_add", "merge_sub"):
        st, rng = step(name, "add")
        a = mk_add(rng, 3, 150, idx_range=40, sigma=True)
        xs = [mk_add(rng, 2, 40, sigma=True), a, mk_add(rng, 3, 300, idx_range=8, sigma=True),
              mk_add(rng, 4, 260, idx_range=20, sigma=True, noncanon=0.5)]
        ys = [mk_add(rng, 3, 40, sigma=True), a, mk_add(rng, 2, 200, idx_range=8, sigma=True),
              mk_add(rng, 1, 90, idx_range=20, sigma=True, noncanon=0.5)]
        add_model(ctx, st, xs, ys, name == "merge_sub", True)
        st.inp.update(xs=xs, ys=ys)
        st.aux.update(over=[False, True, True, True])

    # ---- ct_sum / ct_lincomb
    st, rng = step("sum_routes", "lincomb")      # wave terms, workgroup terms, a scaled segment: all one pass
    pool = [family(rng, 40), family(rng, 70), family(rng, 12), family(rng, 65), family(rng, 33), family(rng, 200)]
    segs = [[0, 2], [1], [3, 4, 2], [5, 0], [4, 1]]
    flags = np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, 0], np.uint32)
    scales = [7, 7, 7, 7, 7, 7, P - 1, (1 << 128) - 1, 12345678901234567890123, 7]
    lincomb_model(ctx, st, pool, segs, scales, flags)
    st.inp.update(pool=pool)
    st, rng = step("sum_fold", "lincomb")        # over the budget (1), out of contract (2), one pass (0)
    two = lambda n, lid: Cipher(mk_add(rng, 2, 1).layers, pack_meta(lid, rng.integers(0, B, n), rng.integers(0, 2, n)),
                                rng.integers(0, 2**64, n, dtype=np.uint64), rng.integers(0, 2**63, n, dtype=np.uint64))
    stray = two(12, [0, 1, 0, 1, 0, 3, 0, 1, 0, 1, 0, 1])   # an edge names layer 3: the partner's second layer
    pool = [lm.strip(c) for c in (mk_add(rng, 2, 50), mk_add(rng, 3, 45), mk_add(rng, 2, 40))] + [stray, two(9, [0] * 9)]
    lincomb_model(ctx, st, pool, [[0, 1, 2], [3, 4], [2, 0], [1]], status=[1, 2, 0, 0])
    st.inp.update(pool=pool)
    st, rng = step("sum_deep", "lincomb", limit=LIMIT_DEEP)   # a term of 30,001 layers
    pool = [family(rng, 30001), family(rng, 40), family(rng, 70)]
    lincomb_model(ctx, st, pool, [[1, 0], [2, 1]])
    st.inp.update(pool=pool)

    # ---- compact: the batched kernel and the merge route
    st, rng = step("compact_routes", "compact")
    cs = [mk_add(rng, 3, 300, idx_range=8, sigma=True), mk_add(rng, 2, 260, idx_range=20, sigma=True, noncanon=0.5),
          mk_add(rng, 21, 200, idx_range=50, sigma=True), mk_add(rng, 22, 200, idx_range=50, sigma=True),
          mk_add(rng, 3, 0, sigma=True)]
    st.inp.update(cs=cs)
    st.out = [rm.compact(oracle, c) for c in cs]
    st.want.update(out=st.out)
    cls = [compact_class(c) for c in cs]
    st.route = {"compact.small": cls.count("small"), "compact.merge": cls.count("merge")}
    st.size = sum(c.nE + c.nL for c in cs)

    # ---- ct_recrypt: a pool of 4
    st, rng = step("recrypt", "recrypt")
    u = lambda nl, ne: _uniform_sigma(rng, mk_add(rng, nl, ne))
    cs = [u(2, 39), _skew(u(2, 39), 8), _skew(u(2, 39), 39), _skew(u(3, 65), 5), u(2, 0)]
    cs[2].sigma[:] = 0
    pool = [u(2, 39 + j) for j in range(4)]
    picks = rng.integers(0, 2**64, (len(cs), 8), dtype=np.uint64)
    res = [recrypt_one(oracle, c, pool, picks[i], k["ubk_inv"], BUDGET["main"]) for i, c in enumerate(cs)]
    st.inp.update(cs=cs, pool=pool, picks=picks)
    st.out = [r[0] for r in res]
    st.want.update(out=st.out, iters=[r[1] for r in res])
    cls = [compact_class(r[2]) for r in res if r[2] is not None]   # a cipher without edges is returned as it came
    st.route = {"compact.small": cls.count("small"), "compact.merge": cls.count("merge")}
    st.size = sum(c.nE + c.nL for c in cs)

    # ---- the smaller operations
    enc = [read_ct(os.path.join(REF, f"enc{i}.ct"))[0] for i in range(4)]
    st, rng = step("commit", "commit_image")
    cs = enc[:3] + [_plain(rng, 3, 70, M_BITS)]
    st.inp.update(cs=cs)
    commit_image_model(ctx, st, cs, True)
    st, rng = step("image", "commit_image")      # weights only: nbits = 0, the 8-byte path
    cs = [lm.strip(c) for c in (enc[3], mk_add(rng, 5, 33), mk_add(rng, 1, 1))]
    st.inp.update(cs=cs)
    commit_image_model(ctx, st, cs, False)
    st, rng = step("gather", "gather")           # select, then cat with a second source
    x1, x2 = [_plain(rng, 1 + i % 3, 10 + 7 * i, M_BITS) for i in range(5)], [_plain(rng, 2, 20 + i, M_BITS) for i in range(2)]
    idx = [4, 0, 0, 2]
    st.inp.update(x1=x1, x2=x2, idx=idx)
    st.out = gam.gather([gam.gather([x1], None, idx), x2])
    st.want.update(out=st.out)
    st.route = {"gather.wide": 2, "gather.ciphers": 4 + 6, "gather.tiles": gather_tiles(st.out[:4]) + gather_tiles(st.out)}
    st, rng = step("metrics", "metrics")
    cs = [_plain(rng, 2, ne, M_BITS, first=i) for i, ne in enumerate((1, 40, 65))] + [_plain(rng, 4, 0, M_BITS)]
    st.inp.update(cs=cs)
    st.want.update(hist=np.stack([np.bincount(np.ascontiguousarray(c.sigma).reshape(-1).view(np.uint8), minlength=256)
                                  .astype(np.uint64) for c in cs]),
                   gsum=[gm.layer_gsums(oracle, c, k["powg"]) for c in cs], status=[0] * len(cs))
    st.route = {"metrics.hist_wide": 1, "metrics.gsum_wave": len(cs)}
    st, rng = step("dec", "dec")
    cs = [lm.strip(mk_add(rng, 1 + i, 20 + 9 * i)) for i in range(3)]
    st.inp.update(cs=cs)
    dec_model(ctx, st, cs, dense_off(cs), sum(c.nL for c in cs), seed_of("dec") + 1)
    st, rng = step("enc", "enc")
    vals = rng.integers(0, 2**64, 3, dtype=np.uint64)
    vals[0] = 0
    rnd = rng.integers(0, 2**64, (3, 256), dtype=np.uint64)
    st.inp.update(vals=vals, rnd=rnd)
    st.out = [oracle.enc_value(k["sk"], int(v), r, k["powg"], canon_tag=k["canon_tag"])[0] for v, r in zip(vals, rnd)]
    st.want.update(out=st.out, status=[0] * 3)
    st.route = {"enc.narrow": 3, "enc.sub": 1, "enc.runs": 1}
    for name, s in (("scale", (0x0123456789ABCDEF << 64) | 0xFEDCBA9876543210), ("neg", P - 1)):
        st, rng = step(name, "scale")
        cs = [lm.strip(mk_add(rng, 2, 40 + 9 * (name == "neg"), noncanon=0.3)), lm.strip(mk_add(rng, 5, 3))]
        st.inp.update(cs=cs, s=s, neg=name == "neg")   # neg: through Engine.ct_neg
        st.out = [lm.ct_scale(oracle, c, s) for c in cs]
        st.want.update(out=st.out)
    st, rng = step("chain", "chain")             # ct_mul_chain, depth 3 on 4 ciphers: the oracle's loop
    xs = [mk_mul(rng, 2, 8, dup_ok=False) for _ in range(4)]
    seed, depth = 0xC4A1, 3
    cur, edges = xs, []
    for d in range(depth):
        l_off, _, tl, _ = mul_layout(cur, xs)
        nz = splitmix_stream(seed + d, 0, 2 * tl)     # nonce_seed + 97 * first input of the chunk + step
        cur = [oracle.ct_mul(c, x, nz[2 * (int(o) + c.nL + x.nL):2 * (int(o) + c.nL + x.nL + c.nL * x.nL)],
                             canon_tag=k["canon_tag"], edge_budget=BUDGET["main"]) for c, x, o in zip(cur, xs, l_off)]
        edges.append(sum(c.nE for c in cur))
    st.inp.update(xs=xs, seed=seed, depth=depth)
    st.out = cur
    st.want.update(counts=[c.nE for c in cur], sumdigests=[sumdigest(c) for c in cur], edges=edges, pair_steps=4 * depth)

    # ---- a ct_mul output, capacity-padded, consumed in place
    prod, prods = by["mul_fresh"], by["mul_sigma"]
    st, rng = step("link_add", "add", src="mul_sigma")   # with sigma; its output feeds link_commit_image
    ys = [_plain(rng, 2, (4, 20, 105)[i], M_BITS) for i in range(3)]
    add_model(ctx, st, prods.out, ys, False, True)
    st.inp.update(ys=ys)
    st, rng = step("link_sum", "lincomb", src="mul_fresh")
    lincomb_model(ctx, st, prod.out, [[0, 1], [2, 3, 4], [4]])
    st, _ = step("link_compact", "compact", src="mul_sigma")
    st.out = [rm.compact(oracle, c) for c in prods.out]
    st.want.update(out=st.out)
    cls = [compact_class(c) for c in prods.out]
    st.route = {"compact.small": cls.count("small"), "compact.merge": cls.count("merge")}
    st, _ = step("link_dec", "dec", src="mul_fresh")
    dec_model(ctx, st, prod.out, prod.aux["l_off"], prod.want["layer_slots"], seed_of("link_dec") + 1)
    st, _ = step("link_scale", "scale", src="mul_fresh")
    st.inp.update(s=P - 2, neg=False)
    st.out = [lm.ct_scale(oracle, c, P - 2) for c in prod.out]
    st.want.update(out=st.out)
    st, _ = step("link_commit_image", "commit_image", src="link_add")
    commit_image_model(ctx, st, by["link_add"].out, True)

    # ---- calls the host refuses before it launches anything
    st, rng = step("ref_stale", "ref_stale")     # exec of a plan that a later plan made stale
    st.inp.update(pairs=split([tiny(rng, 5, 5), tiny(rng, 6, 4)]))
    st.refuse = (EINVAL, "ct_mul_exec: plan is not this context's latest ct_mul plan")
    st, rng = step("ref_sizes", "ref_sizes")     # |A| != |B|, at both plans
    st.inp.update(pairs=split([tiny(rng, 5, 5), tiny(rng, 6, 4)]))
    st.refuse = (EINVAL, "_plan: |A| != |B|")
    st, _ = step("ref_layer_limit", "ref_layer_limit")   # add_deep's pair with the layer limit back at its default
    st.inp.update(xs=by["add_deep"].inp["xs"], ys=by["add_deep"].inp["ys"])
    st.refuse = (ENOSYS, "ct_add_exec: > 30000 layers per cipher")
    st, rng = step("ref_lincomb_status", "ref_lincomb_status")   # the status of 3 segments after an exec of 2
    st.inp.update(pool=[family(rng, 3), family(rng, 5)])
    st.refuse = (EINVAL, "ct_lincomb_status: n is not the last exec's")
    st.route = {"lin.one_pass": 2, "lin.wave_terms": 2}
    st, rng = step("ref_mul_status", "ref_mul_status")   # the status of 3 pairs after an exec of 2
    st.inp.update(pairs=split([tiny(rng, 5, 5), tiny(rng, 6, 4)]), nonces=rng.integers(0, 2**63, 2 * 16, dtype=np.uint64))
    st.refuse = (EINVAL, "ct_mul_status: more pairs than the last ct_mul_exec held")
    st.route = {"mul.fresh": 2, "mul.general": 2, "mul.redo": 2}   # tiny pairs: dynamic chains, no iblk

    # ---- the wide set's two other steps
    st, rng = step("mul_wide", "mul", pset="wide")   # above 120 edges, in hash order at this budget
    mul_model(ctx, st, *split([(lm.strip(mk_add(rng, 2, 40)), lm.strip(mk_add(rng, 2, 39))), general(rng),
                             (lm.strip(mk_add(rng, 2, 37)), lm.strip(mk_add(rng, 2, 40)))]), seed_of("mul_wide") + 1)
    st.want["status"] = [0] * 3
    st, rng = step("link_add_wide", "add", pset="wide", src="mul_wide")
    ys = [lm.strip(mk_add(rng, 2, 30 + i)) for i in range(3)]
    add_model(ctx, st, by["mul_wide"].out, ys, True, False)
    st.inp.update(ys=ys)

    st, rng = step("mul_direct", "mul", pset="wide")   # test_direct_cancelling_key_redo_vs_oracle's batch of 3
    xs = [mk_layers(rng, [674] * 4) for _ in range(3)]   # 4 saturated A layers: no two key slots share a bucket
    ys = [mk_layers(rng, [20, 20]) for _ in range(3)]
    cancel_direct(xs[1], ys[1])
    mul_model(ctx, st, xs, ys, seed_of("mul_direct") + 1, redo=[1])
    st.want["status"] = [0] * 3
    st.aux["cancel"] = 1

    for pset, steps in T.items():
        assert sorted(s.name for s in steps) == sorted(STEP_NAMES[pset]), pset
        for s in steps:
            if not s.size:
                s.size = sum(c.nE + c.nL for c in s.out or s.want.get("out", s.inp.get("cs", [])))
        steps.sort(key=lambda s: STEP_NAMES[pset].index(s.name))
    return T


_TABLE = {}


def table(oracle):
    """build(), once per process."""
    if "T" not in _TABLE:
        _TABLE["T"] = build(oracle)
    return _TABLE["T"]


# ---------------------------------------------------------------------------------------- comparing
def same_value(a, b):
    """Exact equality of two expectation values: ciphers field by field (sigma rows where either has them),
    arrays element by element, the rest by ==."""
    if isinstance(a, Cipher) or isinstance(b, Cipher):
        sg = a.sigma is not None or b.sigma is not None
        if sg and (a.sigma is None or b.sigma is None):
            return False
        return lm.same(a, b, sigma=sg and a.nE > 0)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and bool(np.array_equal(a, b))
    return a == b


# ---------------------------------------------------------------------------------------- orders
def producers(steps):
    return {s.name: s.src for s in steps}


def closed(names, steps):
    """names with every producer moved in front of its first consumer."""
    src, out = producers(steps), []

    def emit(n):
        if n in out:
            return
        if src[n]:
            emit(src[n])
        out.append(n)

    for n in names:
        emit(n)
    return out


def topo_shuffle(steps, seed):
    """A seeded shuffle that keeps every producer before its consumers and is otherwise free."""
    rng = np.random.default_rng(seed)
    src, left, done, out = producers(steps), [s.name for s in steps], set(), []
    while left:
        ready = [n for n in left if not src[n] or src[n] in done]
        n = ready[int(rng.integers(0, len(ready)))]
        left.remove(n)
        done.add(n)
        out.append(n)
    return out


def large_then_small(steps):
    """Every operation's largest step, then at once its smallest (among the steps that need no producer, so
    that nothing comes between the two), then the rest in table order."""
    first = []
    for op in dict.fromkeys(s.op for s in steps):
        mine = [s for s in steps if s.op == op and not s.refuse and not s.src]
        if len(mine) >= 2:
            first += [max(mine, key=lambda s: s.size).name, min(mine, key=lambda s: s.size).name]
    return closed(first + [s.name for s in steps], steps)


ORDERS = ["table", "reverse", "large_small", "shuffle1", "shuffle2", "shuffle3", "shuffle4"]


def order_of(steps, which):
    names = [s.name for s in steps]
    if which == "table":
        return names
    if which == "reverse":
        return closed(names[::-1], steps)
    if which == "large_small":
        return large_then_small(steps)
    return topo_shuffle(steps, 0x5EC0 + int(which[-1]))
