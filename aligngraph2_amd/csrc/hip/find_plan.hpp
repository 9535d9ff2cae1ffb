// find_plan.hpp — the host half of pag_find_all_batch (k_find.hip): the sequences' descriptors are checked and the searched
// offsets are cut into tiles.  Plain C++ without a HIP call, so that tests/harness/find_plan_main.cpp runs it under the address
// and undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>

#include <vector>

namespace pagdev {

constexpr uint32_t FIND_TILE = 1024;  // offsets of one tile: 64 lanes x 16 consecutive offsets

// One wave's work: FIND_TILE offsets (fewer in a sequence's last tile) of one sequence in one strand.  at: the tile's first
// offset, a multiple of FIND_TILE, | 1 when the sequence is searched in its reverse strand.
struct FindTile {
    uint32_t seq, at;
};

struct FindPlan {
    std::vector<FindTile> tiles;     // sequence after sequence, a sequence's tiles in ascending offset
    std::vector<uint64_t> seq_tile;  // [n_seqs + 1] first tile of every sequence
    const char *why = "";            // what check() refused
    uint64_t bad = 0;                // ... and in which sequence
};

// searched offsets of a sequence of len bases: 0 .. len - k
inline uint64_t find_offsets(uint32_t len, uint32_t k) { return len >= k ? (uint64_t)len - k + 1 : 0; }
inline uint64_t find_tiles_of(uint32_t len, uint32_t k) { return (find_offsets(len, k) + FIND_TILE - 1) / FIND_TILE; }

// Every sequence starts on a 4-byte boundary of `packed` and ends inside its packed_bytes (the kernels read up to 12 bytes
// behind a sequence's last byte: the padding pag_seqs promises, which the call's device copy has of its own).
inline bool find_check(const uint64_t *byte_off, const uint32_t *len, uint64_t n_seqs, uint64_t packed_bytes, FindPlan *p) {
    for (uint64_t i = 0; i < n_seqs; ++i) {
        const uint64_t bytes = ((uint64_t)len[i] + 3) / 4;
        p->bad = i;
        if (byte_off[i] & 3u) {
            p->why = "byte_off is not a multiple of 4";
            return false;
        }
        if (byte_off[i] > packed_bytes || bytes > packed_bytes - byte_off[i]) {
            p->why = "the sequence lies beyond packed_bytes";
            return false;
        }
    }
    p->bad = 0;
    return true;
}

// reverse: [n_seqs] or null (all forward).  k in 1 .. 16.
inline void find_cut(const uint32_t *len, const uint8_t *reverse, uint64_t n_seqs, uint32_t k, FindPlan *p) {
    uint64_t n = 0;
    p->seq_tile.assign(n_seqs + 1, 0);
    for (uint64_t i = 0; i < n_seqs; ++i) {
        p->seq_tile[i] = n;
        n += find_tiles_of(len[i], k);
    }
    p->seq_tile[n_seqs] = n;
    p->tiles.resize(n);
    for (uint64_t i = 0; i < n_seqs; ++i) {
        const uint32_t strand = reverse && reverse[i] ? 1u : 0u;
        const uint64_t first = p->seq_tile[i], count = p->seq_tile[i + 1] - first;
        for (uint64_t t = 0; t < count; ++t) p->tiles[first + t] = FindTile{(uint32_t)i, (uint32_t)(t * FIND_TILE) | strand};
    }
}

}  // namespace pagdev
