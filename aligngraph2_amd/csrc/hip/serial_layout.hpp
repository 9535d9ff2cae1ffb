// serial_layout.hpp — where the records of one owner land when its received streams are gathered from several extractions: the
// read ranges of a serial-rank run (pag_shard_run_serial, shard_serial.hip) or the chunks of the ranks of a sharded build
// (pag_shard_run, shard_comm.hip).  Plain C++, no device code: tests/harness/serial_layout_test.cpp drives it on the CPU.
//
// counts[(r * n_owners + o) * 4 + q]: what read range r of n_ranges sends owner o — q = 0 tuples of pass 1, 1 tuples of pass 2,
// 2 edges of pass 1, 3 edges of pass 2 (the layout of pag_shard_extract's `counts`, one row per range).  An owner builds from
//     [pass 1 from range 0] .. [pass 1 from range n-1] [pass 2 from range 0] .. [pass 2 from range n-1]
// (include/pagraph_hip.h, pag_shard_*: the canonical order of a k-mer's records), tuples and edges each in a buffer of their own.
// A serial-rank run has as many ranges as owners; the C chunks of W ranks, rank-major (chunk_range), are W * C ranges for W owners.
#pragma once
#include <cstdint>
#include <vector>

namespace pagdev {

struct OwnerLayout {
    uint64_t n_t = 0, t1 = 0;  // tuples the owner receives, of which pass 1 (they come first)
    uint64_t n_e = 0, e1 = 0;  // edges likewise
};

// sizes of owner o's receive buffers
inline OwnerLayout owner_layout(const uint64_t *counts, uint32_t n_ranges, uint32_t n_owners, uint32_t o) {
    OwnerLayout L;
    for (uint32_t r = 0; r < n_ranges; ++r) {
        const uint64_t *c = counts + ((uint64_t)r * n_owners + o) * 4;
        L.t1 += c[0];
        L.n_t += c[0] + c[1];
        L.e1 += c[2];
        L.n_e += c[2] + c[3];
    }
    return L;
}

struct RangeSlots {
    uint64_t t_at1 = 0, t_at2 = 0;  // first slot of range r's pass-1 / pass-2 tuples in the owner's tuple buffer
    uint64_t e_at1 = 0, e_at2 = 0;  // ... of its edges in the owner's edge buffer
};

// where range r's records of owner o go
inline RangeSlots range_slots(const uint64_t *counts, uint32_t n_ranges, uint32_t n_owners, uint32_t o, uint32_t r) {
    const OwnerLayout L = owner_layout(counts, n_ranges, n_owners, o);
    RangeSlots S;
    S.t_at2 = L.t1;
    S.e_at2 = L.e1;
    for (uint32_t q = 0; q < r; ++q) {
        const uint64_t *c = counts + ((uint64_t)q * n_owners + o) * 4;
        S.t_at1 += c[0];
        S.t_at2 += c[1];
        S.e_at1 += c[2];
        S.e_at2 += c[3];
    }
    return S;
}

// (n ranges for n owners as callers written before the chunked receive spell it — the harness of an earlier tests/ must still build; new code passes both)
inline OwnerLayout owner_layout(const uint64_t *counts, uint32_t n, uint32_t o) { return owner_layout(counts, n, n, o); }
inline RangeSlots range_slots(const uint64_t *counts, uint32_t n, uint32_t o, uint32_t r) { return range_slots(counts, n, n, o, r); }

// The same stretches in the streams pag_shard_extract_range leaves partitioned by owner ([owner 0: pass 1, pass 2] [owner 1: ..]):
// where owner o's pass-1 / pass-2 records of range r start there (what pag_shard_take_part is asked for).
inline RangeSlots partitioned_slots(const uint64_t *counts, uint32_t n_owners, uint32_t o, uint32_t r) {
    RangeSlots S;
    const uint64_t *row = counts + (uint64_t)r * n_owners * 4;
    for (uint32_t q = 0; q < o; ++q) {
        S.t_at1 += row[q * 4 + 0] + row[q * 4 + 1];
        S.e_at1 += row[q * 4 + 2] + row[q * 4 + 3];
    }
    S.t_at2 = S.t_at1 + row[o * 4 + 0];
    S.e_at2 = S.e_at1 + row[o * 4 + 2];
    return S;
}

// ---- a sharded build: every rank sends its read range in C chunks, chunk ch of all ranks in one exchange; chunk ch of `rank` is range
inline uint32_t chunk_range(uint32_t rank, uint32_t C, uint32_t ch) { return rank * C + ch; }
// both passes' records of one stream (0 tuples, 1 edges) that range r sends owner o: what travels together
inline uint64_t range_records(const uint64_t *counts, uint32_t n_owners, uint32_t r, uint32_t o, uint32_t stream) {
    const uint64_t *c = counts + ((uint64_t)r * n_owners + o) * 4 + 2 * stream;
    return c[0] + c[1];
}

// The copies that put what owner o received of one stream into its buffer, in records.  A chunk's receive array is, as the
// exchange fills it, [from rank 0: pass 1, pass 2][from rank 1: ..]; the buffer is [pass 1: rank 0 chunk 0, chunk 1, .. rank 1 ..]
// [pass 2: likewise] — the order above with the ranges chunk_range names.  n, n1: the buffer's records and its pass-1 records
// (OwnerLayout's n_t, t1 or n_e, e1).
struct ReceivePlan {
    struct Copy {
        uint32_t chunk;        // out of this chunk's receive array
        uint64_t src, dst, n;  // first record there / in the owner's buffer; how many
    };
    uint64_t n = 0, n1 = 0;
    std::vector<Copy> copies;  // (none of them empty)
};
inline ReceivePlan chunked_receive_plan(const uint64_t *counts, uint32_t W, uint32_t C, uint32_t o, uint32_t stream) {
    const OwnerLayout L = owner_layout(counts, W * C, W, o);
    ReceivePlan P;
    P.n = stream ? L.n_e : L.n_t;
    P.n1 = stream ? L.e1 : L.t1;
    std::vector<uint64_t> src(C);  // read position in every chunk's receive array
    uint64_t dst[2] = {0, P.n1};
    for (uint32_t rank = 0; rank < W; ++rank)
        for (uint32_t ch = 0; ch < C; ++ch)
            for (uint32_t pass = 0; pass < 2; ++pass) {
                const uint64_t n = counts[((uint64_t)chunk_range(rank, C, ch) * W + o) * 4 + 2 * stream + pass];
                if (n) P.copies.push_back({ch, src[ch], dst[pass], n});
                src[ch] += n;
                dst[pass] += n;
            }
    return P;
}

}  // namespace pagdev
