// cns_device.hpp — what the two device forms of pa_cns's graph stage share (k_cns.hip: a part per wavefront run by one lane;
// k_cns_wave.hip: a part per wavefront with the lanes on the columns of an alignment and the levels of bestPath): the host loop
// that uploads the inputs, cuts the parts into batches whose graph regions fit the device memory budget and launches one
// kernel per batch.
#pragma once
#include "cns_graph.hpp"
#include "pag_device.hpp"

namespace pagdev {

// one batch: n parts (parts[] is device memory, their regions inside A), one wavefront per part
using CnsLaunchFn = void (*)(const pagcns::Arrays &A, const pagcns::Part *parts, uint32_t n, const char *backbone, const pagcns::Aln *alns, const char *qpool,
                             const char *tpool, int min_weight, char *out, uint32_t *out_len, int32_t *part_err);

// the body of pag_cns_consensus / pag_cns_consensus_wave (include/pagraph_hip.h); `who` names the entry point in errors.
// d_qpool / d_tpool: the pools in device memory already (pag_cns_consensus_rows) — qpool / tpool are not read then
int cns_consensus_batched(const char *who, CnsLaunchFn launch, int device, const char *backbone, uint64_t backbone_len, const pag_cns_part *parts, uint64_t n_parts,
                          const pag_cns_aln *alns, uint64_t n_alns, const char *qpool, const char *tpool, uint64_t pool_bytes, int32_t min_weight, char *out,
                          uint64_t out_bytes, uint64_t *out_off, uint32_t *out_len, int32_t *part_err, const char *d_qpool = nullptr,
                          const char *d_tpool = nullptr);
// the two launchers (k_cns.hip: a lane per part; k_cns_wave.hip: a wavefront per part)
CnsLaunchFn cns_launcher_lane();
CnsLaunchFn cns_launcher_wave();

}  // namespace pagdev
