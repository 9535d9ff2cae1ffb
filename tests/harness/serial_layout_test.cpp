// tests/harness/serial_layout_test.cpp — test-only.
// C wrappers over the offset arithmetic of a serial-rank run (aligngraph2_amd/csrc/hip/serial_layout.hpp) so that
// tests/test_serial_layout.py can hold it against a numpy restatement without a GPU.  Built by the host compiler alone: that
// this file compiles is the proof that the header has no device code in it.
#include <cstdint>

#include "serial_layout.hpp"

extern "C" {

// out: n_t, t1, n_e, e1
void pagt_owner_layout(const uint64_t *counts, uint32_t n, uint32_t o, uint64_t *out) {
    const pagdev::OwnerLayout L = pagdev::owner_layout(counts, n, o);
    out[0] = L.n_t;
    out[1] = L.t1;
    out[2] = L.n_e;
    out[3] = L.e1;
}

// out: t_at1, t_at2, e_at1, e_at2
void pagt_range_slots(const uint64_t *counts, uint32_t n, uint32_t o, uint32_t r, uint64_t *out) {
    const pagdev::RangeSlots S = pagdev::range_slots(counts, n, o, r);
    out[0] = S.t_at1;
    out[1] = S.t_at2;
    out[2] = S.e_at1;
    out[3] = S.e_at2;
}

void pagt_partitioned_slots(const uint64_t *counts, uint32_t n, uint32_t o, uint32_t r, uint64_t *out) {
    const pagdev::RangeSlots S = pagdev::partitioned_slots(counts, n, o, r);
    out[0] = S.t_at1;
    out[1] = S.t_at2;
    out[2] = S.e_at1;
    out[3] = S.e_at2;
}

}  // extern "C"
