// query_call.hpp — the host side the on-demand queries over the finished graph share (pag_successors_batch, pag_find_all_batch,
// pag_walk_straight_batch): a call in two passes.  The kernel counts, the counts are scanned into offsets, the offsets and the
// totals go to the host; a caller whose buffers hold the totals gets the second pass, which fills.  What is allocated before the
// counts are known is ONE block, carved by a Carver; the records are allocated between the passes.  ms_kernels is the device time
// between the brackets of the counting pass, and after the filling pass the sum of the two.
#pragma once
#include <algorithm>

#include "dev_call.hpp"
#include "pag_graph_impl.hpp"

namespace pagdev {

// offsets into one block, each array on a 256-byte boundary; `bytes` is the block's size
struct Carver {
    size_t bytes = 0;
    template <typename T>
    size_t take(uint64_t n) {
        const size_t at = bytes;
        bytes += (n * sizeof(T) + 255u) & ~(size_t)255u;
        return at;
    }
};

// The two refusals of a handle the queries cannot answer from; what_a_region_lacks completes "a region does not hold every ...".
inline int check_finished_graph(const pag_graph *g, const char *who, const char *what_a_region_lacks) {
    if (!g->tkey) {
        set_error("%s: the handle holds no finished graph (pag_process / pag_shard_import first)", who);
        return PAG_EINVAL;
    }
    if (g->regional) {
        set_error("%s: the handle holds one rank's region of a block (pag_shard_set_region): a region does not hold every %s", who, what_a_region_lacks);
        return PAG_ERANGE;
    }
    return PAG_OK;
}

// A wave per item, 4 waves per block; more blocks than are resident at once (6 to 8 per CU by the kernels' registers): the
// dispatcher keeps every CU full to the end
inline unsigned wave_per_item_grid(uint64_t n_items) { return (unsigned)std::min<uint64_t>((n_items + 3) / 4, 256u * 32u); }

struct QueryCall : DevCall {  // on the handle's device and stream
    enum Pass { COUNT = 0, FILL = 1 };
    char *block = nullptr;  // what is allocated before the counts are known
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double ms = 0;  // device time of the passes that are done
    explicit QueryCall(const char *w) : DevCall(w) {}
    ~QueryCall() {
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
    }
    int open(const pag_graph *g, size_t block_bytes) {
        s = g->stream;
        int rc = DevCall::open(g->device, false, DevCall::NO_STREAM);
        if (rc || (rc = alloc(&block, block_bytes))) return rc;
        for (hipEvent_t &e : ev) PAG_HIP_TRY(hipEventCreate(&e));
        return PAG_OK;
    }
    template <typename T>
    T *at(size_t offset) const {
        return (T *)(block + offset);
    }
    // the brackets around a pass's kernels ...
    int begin(Pass p) {
        PAG_HIP_TRY(hipEventRecord(ev[2 * p], s));
        return PAG_OK;
    }
    int end(Pass p) {
        PAG_HIP_TRY(hipEventRecord(ev[2 * p + 1], s));
        return PAG_OK;
    }
    // ... and, behind the copies to the host the caller has put on the stream: wait for them; ms_kernels so far
    int done(Pass p, double *ms_kernels) {
        PAG_HIP_TRY(hipStreamSynchronize(s));
        float t = 0;
        PAG_HIP_TRY(hipEventElapsedTime(&t, ev[2 * p], ev[2 * p + 1]));
        ms += (double)t;
        if (ms_kernels) *ms_kernels = ms;
        return PAG_OK;
    }
};

}  // namespace pagdev
