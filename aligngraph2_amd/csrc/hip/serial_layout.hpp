// serial_layout.hpp — where the records of one owner land when its received streams are gathered from several extractions
// (pag_shard_run_serial, shard_serial.hip).  Plain C++, no device code: tests/harness/serial_layout_test.cpp drives it on the CPU.
//
// counts[(r * n + o) * 4 + q]: what read range r sends owner o — q = 0 tuples of pass 1, 1 tuples of pass 2, 2 edges of pass 1,
// 3 edges of pass 2 (the layout of pag_shard_extract's `counts`, one row per range).  An owner builds from
//     [pass 1 from range 0] .. [pass 1 from range n-1] [pass 2 from range 0] .. [pass 2 from range n-1]
// (include/pagraph_hip.h, pag_shard_*: the canonical order of a k-mer's records), tuples and edges each in a buffer of their own.
#pragma once
#include <cstdint>

namespace pagdev {

struct OwnerLayout {
    uint64_t n_t = 0, t1 = 0;  // tuples the owner receives, of which pass 1 (they come first)
    uint64_t n_e = 0, e1 = 0;  // edges likewise
};

// sizes of owner o's receive buffers
inline OwnerLayout owner_layout(const uint64_t *counts, uint32_t n, uint32_t o) {
    OwnerLayout L;
    for (uint32_t r = 0; r < n; ++r) {
        const uint64_t *c = counts + ((uint64_t)r * n + o) * 4;
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
inline RangeSlots range_slots(const uint64_t *counts, uint32_t n, uint32_t o, uint32_t r) {
    const OwnerLayout L = owner_layout(counts, n, o);
    RangeSlots S;
    S.t_at2 = L.t1;
    S.e_at2 = L.e1;
    for (uint32_t q = 0; q < r; ++q) {
        const uint64_t *c = counts + ((uint64_t)q * n + o) * 4;
        S.t_at1 += c[0];
        S.t_at2 += c[1];
        S.e_at1 += c[2];
        S.e_at2 += c[3];
    }
    return S;
}

// The same stretches in the streams pag_shard_extract_range leaves partitioned by owner ([owner 0: pass 1, pass 2] [owner 1: ..]):
// where owner o's pass-1 / pass-2 records of range r start there (what pag_shard_take_part is asked for).
inline RangeSlots partitioned_slots(const uint64_t *counts, uint32_t n, uint32_t o, uint32_t r) {
    RangeSlots S;
    const uint64_t *row = counts + (uint64_t)r * n * 4;
    for (uint32_t q = 0; q < o; ++q) {
        S.t_at1 += row[q * 4 + 0] + row[q * 4 + 1];
        S.e_at1 += row[q * 4 + 2] + row[q * 4 + 3];
    }
    S.t_at2 = S.t_at1 + row[o * 4 + 0];
    S.e_at2 = S.e_at1 + row[o * 4 + 2];
    return S;
}

}  // namespace pagdev
