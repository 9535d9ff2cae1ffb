// tests/harness/serial_layout_test.cpp — test-only.
// C wrappers over the offset arithmetic of a serial-rank run (aligngraph2_amd/csrc/hip/serial_layout.hpp) so that
// tests/test_serial_layout.py can hold it against a numpy restatement without a GPU.  Built by the host compiler alone: that
// this file compiles is the proof that the header has no device code in it.
#include <cstdint>

#include "serial_layout.hpp"

extern "C" {

// (a serial-rank run: as many ranges as owners)
// out: n_t, t1, n_e, e1
void pagt_owner_layout(const uint64_t *counts, uint32_t n, uint32_t o, uint64_t *out) {
    const pagdev::OwnerLayout L = pagdev::owner_layout(counts, n, n, o);
    out[0] = L.n_t;
    out[1] = L.t1;
    out[2] = L.n_e;
    out[3] = L.e1;
}

// out: t_at1, t_at2, e_at1, e_at2
void pagt_range_slots(const uint64_t *counts, uint32_t n, uint32_t o, uint32_t r, uint64_t *out) {
    const pagdev::RangeSlots S = pagdev::range_slots(counts, n, n, o, r);
    out[0] = S.t_at1;
    out[1] = S.t_at2;
    out[2] = S.e_at1;
    out[3] = S.e_at2;
}

void pagt_partitioned_slots(const uint64_t *counts, uint32_t n, uint32_t o, uint32_t r, uint64_t *out) {
    const pagdev::RangeSlots S = pagdev::partitioned_slots(counts, n, o, r);  // (a row has one entry per owner)
    out[0] = S.t_at1;
    out[1] = S.t_at2;
    out[2] = S.e_at1;
    out[3] = S.e_at2;
}

// The copy plan of a chunked receive: counts[(rank * C + chunk) * W + owner][4]; stream 0 tuples, 1 edges.  sizes: n, n1;
// copies[i * 4 ..]: chunk, source offset in that chunk's receive array, destination offset, count — the first `cap` of them.
// Returns how many copies the plan has.
uint64_t pagt_chunked_receive_plan(const uint64_t *counts, uint32_t W, uint32_t C, uint32_t o, uint32_t stream, uint64_t *sizes, uint64_t *copies, uint64_t cap) {
    const pagdev::ReceivePlan P = pagdev::chunked_receive_plan(counts, W, C, o, stream);
    sizes[0] = P.n;
    sizes[1] = P.n1;
    for (uint64_t i = 0; i < P.copies.size() && i < cap; ++i) {
        copies[i * 4 + 0] = P.copies[i].chunk;
        copies[i * 4 + 1] = P.copies[i].src;
        copies[i * 4 + 2] = P.copies[i].dst;
        copies[i * 4 + 3] = P.copies[i].n;
    }
    return P.copies.size();
}

}  // extern "C"
