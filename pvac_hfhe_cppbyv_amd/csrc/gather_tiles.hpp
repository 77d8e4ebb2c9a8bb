// gather_tiles.hpp — the work split of pvac_hip_batch_gather (k_gather.hip, rt_gather.cpp): the tile
// geometry of a sigma width, the tiles of one cipher, the tile -> cipher search, the runs of tiles dealt
// to lane groups and the head / body / tail split of a 16-byte copy. Pure integer arithmetic: no HIP
// runtime calls and no other header of the library, so it is checked without a GPU
// (tests/cpp/gather_tiles_check.cpp). The kernel and the runtime call the same functions, so what the
// check proves is what runs.
//
// Terms. A TILE is at most ept consecutive edge rows of one output cipher, or at most lpt consecutive
// layer records of one. A cipher of E edges and L layers has te = ceil(E / ept) edge tiles followed by
// tl = ceil(L / lpt) layer tiles; a cipher without rows has none. Tiles are numbered through the output:
// toff = the exclusive scan of the per-cipher tile counts, tile t belongs to the last cipher k with
// toff[k] <= t. A lane GROUP (a wave, or a whole workgroup) copies one tile at a time and takes a RUN
// of consecutive tiles, so it searches once and then only walks forward.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PVHIP_GATHER_FN __host__ __device__ inline
#else
#define PVHIP_GATHER_FN inline
#endif

namespace pvhip {

constexpr uint32_t kGatherTileBytes = 16384;   // an edge tile moves at most this many bytes (the codec's kCtTileBytes)
constexpr uint32_t kGatherLayerBytes = 40;     // sizeof(pvac_layer): five 8-byte words
constexpr uint32_t kGatherBlock = 256;         // threads per workgroup
constexpr uint32_t kGatherBlocksPerCu = 8;     // the grid's cap: full occupancy of an LDS-free kernel

struct gather_geom {
    uint32_t ept, lpt;   // edge rows per tile, layer records per tile
};

// an edge row is meta, w_lo, w_hi and sigma_words words of sigma (0: weights only)
PVHIP_GATHER_FN uint64_t gather_edge_bytes(uint32_t sigma_words) { return 24ull + 8ull * sigma_words; }

PVHIP_GATHER_FN gather_geom gather_geom_of(uint32_t sigma_words) {
    gather_geom g;
    const uint64_t e = kGatherTileBytes / gather_edge_bytes(sigma_words);
    g.ept = e ? (uint32_t)e : 1u;
    g.lpt = kGatherTileBytes / kGatherLayerBytes;
    return g;
}

PVHIP_GATHER_FN uint64_t gather_div_up(uint64_t a, uint32_t b) { return a / b + (a % b ? 1u : 0u); }

// tiles of a cipher of E edges and L layers
PVHIP_GATHER_FN uint64_t gather_tiles(uint64_t E, uint64_t L, const gather_geom& g) {
    return gather_div_up(E, g.ept) + gather_div_up(L, g.lpt);
}

// Tile t (< gather_tiles) of a cipher: its kind and its rows [first, first + count).
struct gather_piece {
    bool layers;          // false: edge rows, true: layer records
    uint64_t first, count;
};
PVHIP_GATHER_FN gather_piece gather_piece_of(uint64_t E, uint64_t L, const gather_geom& g, uint64_t t) {
    gather_piece p;
    const uint64_t te = gather_div_up(E, g.ept);
    p.layers = t >= te;
    const uint64_t rows = p.layers ? L : E;
    const uint32_t per = p.layers ? g.lpt : g.ept;
    p.first = (p.layers ? t - te : t) * per;
    p.count = rows - p.first < per ? rows - p.first : per;
    return p;
}

// largest k < n with toff[k] <= t (n > 0, t below the tile total): ciphers without tiles share an
// offset with their successor and are never found
PVHIP_GATHER_FN uint64_t gather_tile_cipher(const uint64_t* toff, uint64_t n, uint64_t t) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (toff[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// tiles [lo, hi) of group g of `groups`: runs of ceil(ntiles / groups), clipped
PVHIP_GATHER_FN void gather_run(uint64_t ntiles, uint64_t groups, uint64_t g, uint64_t& lo, uint64_t& hi) {
    const uint64_t per = ntiles / groups + (ntiles % groups ? 1u : 0u);
    lo = g * per;
    if (lo > ntiles) lo = ntiles;
    hi = ntiles - lo < per ? ntiles : lo + per;
}

// workgroups for ntiles tiles, tpb lane groups per workgroup: one tile per group up to the cap
PVHIP_GATHER_FN uint64_t gather_grid(uint64_t ntiles, uint32_t tpb, uint32_t num_cus) {
    const uint64_t want = ntiles / tpb + (ntiles % tpb ? 1u : 0u);
    const uint64_t cap = (uint64_t)num_cus * kGatherBlocksPerCu;
    return want < cap ? want : cap;
}

// The copy of n 8-byte words from word address s to word address d (byte address / 8). Where the two
// have the same parity, an odd d takes one 8-byte head word, then `pairs` 16-byte pieces start at an
// even word on both sides, then at most one 8-byte tail word; where they differ every word goes alone
// (head = n). head + 2 pairs + tail == n, and no piece reaches outside [0, n).
struct gather_split {
    uint64_t head, pairs, tail;
};
PVHIP_GATHER_FN gather_split gather_split_of(uint64_t s, uint64_t d, uint64_t n) {
    gather_split p;
    if ((s ^ d) & 1u) {
        p.head = n;
        p.pairs = p.tail = 0;
        return p;
    }
    p.head = n && (d & 1u) ? 1u : 0u;
    p.pairs = (n - p.head) / 2;
    p.tail = (n - p.head) & 1u;
    return p;
}

// sigma rows of sigma_words words move 16 bytes at a time when every row of both sides starts on a
// 16-byte boundary: an even row width and 16-byte-aligned bases (low address bits OR-ed over the sides)
PVHIP_GATHER_FN bool gather_sigma_wide(uint32_t sigma_words, uint64_t base_bits) {
    return sigma_words && !(sigma_words & 1u) && !(base_bits & 15u);
}

}  // namespace pvhip
