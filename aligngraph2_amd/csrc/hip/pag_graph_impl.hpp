// Internal: the handle behind include/pagraph_hip.h and its pooled device buffers.
#pragma once
#include <algorithm>
#include <chrono>
#include <vector>

#include "pag_device.hpp"
#include "pag_travel.hpp"
#include "pool_slots.hpp"

namespace pagdev {
// A buffer the handle owns outside the pool: one allocation, replaced (never copied) when it is too small.
struct OwnedBuf {
    enum Kind : uint8_t { DEVICE, PINNED, PINNED_MAPPED };  // hipMalloc; hipHostMalloc default; coherent + mapped
    void *p = nullptr;
    size_t cap = 0;
    Kind kind = DEVICE;
    explicit OwnedBuf(Kind k = DEVICE) : kind(k) {}
    static void free_raw(void *q, Kind k) {
        if (!q) return;
        if (k == DEVICE) hipFree(q);
        else hipHostFree(q);
    }
    // room for `need` bytes: a buffer that has them stays, any other is replaced by one of `want` bytes (its contents are
    // dropped; under g->defer_free the old one is parked in g->deferred).  After a failure the buffer is empty.
    inline hipError_t grow(pag_graph *g, size_t need, size_t want);
    void release() {
        free_raw(p, kind);
        p = nullptr;
        cap = 0;
    }
    template <typename T>
    T *as() const {
        return (T *)p;
    }
};
}  // namespace pagdev

struct pag_graph {
    using OwnedBuf = pagdev::OwnedBuf;
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t k = 0;
    uint64_t n_solid = 0;
    int all_solid = 0;
    uint32_t *solid_bits = nullptr;  // 4^k bits
    // finished graph (device): k-mer-sorted streams with in-place segment results
    uint64_t n_t = 0, n_e = 0;
    uint32_t *tkey = nullptr;
    uint64_t *tval = nullptr;
    uint32_t *tseg = nullptr;
    uint16_t *tcnt = nullptr;
    uint32_t *ekey = nullptr;
    uint64_t *eval = nullptr;
    uint32_t *eseg = nullptr;
    pag_build_stats stats{};
    // pag_shard_extract -> pag_shard_take: sizes of the partitioned streams (tuples, edges) and which buffer of each
    // ping-pong pair holds them
    uint64_t shard_x[2] = {0, 0};
    int shard_in0[2] = {1, 1};
    // a serial-rank run (pag_shard_run_serial, shard_serial.hip): what turn 0 found — counts[(r * n + o) * 4 + q], the records
    // read range r sends owner o, and the block's count lines — held against every later turn of the block
    struct SerialRun {
        bool valid = false;
        uint32_t n = 0;
        std::vector<uint64_t> counts;
        pag_build_stats total{};
    } serial;
    // device memory pool: every buffer of the pipeline lives in a named slot (the registry: pool_slots.hpp) that is reused
    // (and only ever grown) across pag_process calls, so steady-state calls do no hipMalloc/hipFree at all
    struct Slot {
        void *p = nullptr;
        size_t cap = 0;
    };
    Slot pool[pagdev::ps::COUNT];
    // what the pool cost (PAGRAPH_TIMING reports it per stage: at the sizes of BASELINE configs[2] / [3] a fresh handle's tens of
    // GB are seconds of hipMalloc / hipFree)
    double alloc_ms = 0;
    uint64_t alloc_bytes = 0, alloc_calls = 0;
    // per-contig walker buffers (k5_travel_host.hip), grown on demand like the slots above
    std::vector<Slot> cpool;
    // while the persistent walker is resident nothing may be freed, device or pinned memory (either synchronises the device):
    // replaced buffers are parked here and released afterwards (drain_deferred)
    bool defer_free = false;
    struct Parked {
        void *p;
        OwnedBuf::Kind kind;
    };
    std::vector<Parked> deferred;
    // job queue of the persistent walker (fine-grained host memory) and its device-side ticket counter
    OwnedBuf wq_host{OwnedBuf::PINNED_MAPPED}, wq_next;
    std::vector<hipStream_t> walk_streams;  // the walker launches' streams (WalkerGrid, walker_grid.hpp)
    // traversal state (k5_travel_host.hip)
    pagdev::TravGraph tg{};
    bool tg_ready = false;
    uint64_t tg_dev = 0;   // parameters the successor records were built with
    double tg_err = 0;
    // result of the last pag_travel: one array in pinned host memory (grown, never released before pag_destroy), slot
    // 2 * contig + (reverse ? 1 : 0) at path_off / path_len
    OwnedBuf path_store{OwnedBuf::PINNED};
    std::vector<uint64_t> path_off, path_len;
    hipStream_t deliver_stream = nullptr;  // copies of finished contigs' paths while the walks run (pag_travel)
    std::vector<const pag_path_node *> path_ptr;  // non-null: the orientation's path, delivered while the walks ran (pinned fetch memory)
    std::vector<uint8_t> path_valid;  // that orientation was traversed by the last pag_travel
    // the dump text of the delivered paths (PAG_TRAVEL_RENDER_DUMPS; pinned fetch memory like path_ptr) and the device memory
    // the renderings use: the PositionMapper tables, the scratch of the epilogue's renderings
    std::vector<const char *> text_ptr;
    std::vector<uint64_t> text_len;
    // ... and their consensus sequences (PAG_TRAVEL_RENDER_SEQS, k5_seq.hip); seq_refs: the references' bases as
    // pag_travel_seq_sources left them for the next pag_travel
    std::vector<const char *> seq_ptr;
    std::vector<uint64_t> seq_len;
    const pag_seqs *seq_refs = nullptr;
    OwnedBuf dump_tables, dump_scratch;
    // device arena of the walker's job buffers (bump pointer, reset by every pag_travel)
    OwnedBuf walk_arena;
    size_t walk_arena_used = 0;
    std::vector<OwnedBuf> fetch_chunks;  // pinned chunks for the paths fetched from the walker (pag_travel)
    // the graph holds only a region of the block (pag_shard_set_region after pag_shard_import): the reference bands of its
    // coordinate-free vertices, [lo, hi) pairs sorted, and which ends are open (the block goes on beyond them, on other ranks)
    bool regional = false;
    std::vector<uint32_t> region_ref_iv;
    std::vector<uint8_t> region_ref_open;
    // the traversal view (g->tg) was built for these orientations only (trav_view_region, k5_travel_host.hip): it leaves out
    // what no traversal of them can examine.  view_off: a walk did leave the view (pag_travel then rebuilds the whole graph's
    // view and walks again); both are reset with the graph.
    bool view_pruned = false, view_off = false;
    std::vector<int32_t> view_orient;
    uint64_t view_counts[3] = {0, 0, 0};  // nodes, vertices, edges of the view
    uint64_t view_fallbacks = 0;          // (since the handle was created)
    double succ_per_vertex = 3.0;  // emission-stream slots per vertex of the last traversal graph: sizes the stream of the next (trav_prepare_graph)
    uint64_t n_zero_ctg = 0;  // new ids below it: vertices without a contig coordinate, in reference-coordinate order
    // pinned host staging area of the traversal (packed job results, uploads)
    OwnedBuf pin_host{OwnedBuf::PINNED};
    // debug: raw emitted streams (host copies), kept when PAG_DEBUG_KEEP_STREAMS=1
    std::vector<uint32_t> dbg_tkey, dbg_ekey;
    std::vector<uint64_t> dbg_tval, dbg_eval;
};


namespace pagdev {

// what the walker's residency parked (pag_graph::deferred) is released; the caller knows the grid is down
inline void drain_deferred(pag_graph *g) {
    g->defer_free = false;
    for (const pag_graph::Parked &q : g->deferred) OwnedBuf::free_raw(q.p, q.kind);
    g->deferred.clear();
}
// an allocation of the handle that is no longer wanted: freed, or parked while nothing may be freed
inline void retire(pag_graph *g, void *p, OwnedBuf::Kind kind) {
    if (!p) return;
    if (g->defer_free) g->deferred.push_back({p, kind});
    else OwnedBuf::free_raw(p, kind);
}
inline hipError_t OwnedBuf::grow(pag_graph *g, size_t need, size_t want) {
    if (cap >= need) return hipSuccess;
    retire(g, p, kind);
    p = nullptr;
    cap = 0;
    const hipError_t e = kind == DEVICE ? hipMalloc(&p, want) : hipHostMalloc(&p, want, kind == PINNED ? hipHostMallocDefault : hipHostMallocCoherent | hipHostMallocMapped);
    if (e != hipSuccess) p = nullptr;
    else cap = want;
    return e;
}
// one more pinned chunk for the fetched paths (pag_reserve_walk_arena ahead of the walks, fetch_alloc when they need one)
inline void *fetch_chunk_add(pag_graph *g, size_t bytes) {
    OwnedBuf c(OwnedBuf::PINNED);
    if (c.grow(g, bytes, bytes) != hipSuccess) return nullptr;
    g->fetch_chunks.push_back(c);
    return c.p;
}

inline void slot_free(pag_graph *g, pag_graph::Slot &sl) {
    retire(g, sl.p, OwnedBuf::DEVICE);
    sl.p = nullptr;
    sl.cap = 0;
}
// The one way a pool slot grows.  A slot that holds `need` bytes stays as it is; any other is replaced by an array of `want`
// bytes (each caller's own formula) whose first `keep_bytes` are the old array's.  The allocation is booked in
// alloc_ms / bytes / calls.
//   keep_bytes == 0: the old array goes first, so the peak is one array — after a failed allocation the slot is empty.
//   keep_bytes != 0: allocate, copy, then let the old array go — after a failed allocation or copy the slot is as it was.
// The copy is queued on `s` and waited for: it comes after whatever `s` wrote into the old array, which may then be freed.
// (Not a blocking hipMemcpy: that is ordered after other streams' work only when they are blocking streams.)  The callers see to
// it that nothing on ANOTHER stream still uses the old array — shard_comm.hip ends its exchange first; shard_serial.hip has none.
inline int slot_grow(pag_graph *g, pag_graph::Slot &sl, size_t need, size_t want, size_t keep_bytes, hipStream_t s) {
    if (sl.cap >= need) return PAG_OK;
    if (want < need || keep_bytes > sl.cap || keep_bytes > want) {
        set_error("slot_grow: need %zu, want %zu, keep %zu of a slot of %zu bytes", need, want, keep_bytes, sl.cap);
        return PAG_EINVAL;
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (!keep_bytes) slot_free(g, sl);
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, want);
    g->alloc_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g->alloc_bytes += want;
    g->alloc_calls += 1;
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        return PAG_ENOMEM;
    }
    if (keep_bytes) {
        e = hipMemcpyAsync(p, sl.p, keep_bytes, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            hipFree(p);
            set_error("a slot's first %zu bytes could not be moved: %s", keep_bytes, hipGetErrorString(e));
            return PAG_EFAULT;
        }
        slot_free(g, sl);
    }
    sl.p = p;
    sl.cap = want;
    return PAG_OK;
}

struct DevBuf {  // a view of one pool slot of the handle (never frees; pag_destroy does)
    pag_graph *g = nullptr;
    pag_graph::Slot *sl = nullptr;
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(pag_graph *gg, ps::Id s) : g(gg), sl(&gg->pool[s]) {}
    DevBuf(pag_graph *gg, pag_graph::Slot *slot) : g(gg), sl(slot) {}
    int alloc_keeping(size_t bytes, size_t keep_bytes, size_t want) {
        const int rc = slot_grow(g, *sl, bytes, want, keep_bytes, g->stream);
        p = sl->p;
        return rc;
    }
    int alloc(size_t bytes) {
        if (bytes == 0) bytes = 16;
        // (room to grow without another hipMalloc: an eighth, at most 512 MB — an eighth of every slot was 25 GB of a 90 Mb block at 30x)
        return alloc_keeping(bytes, 0, bytes + std::min<size_t>(bytes / 8, (size_t)512 << 20) + 256);
    }
    template <typename T>
    T *as() const {
        return (T *)p;
    }
};


// where the extracted (t_in0 = e_in0 = 1: as extract_stage left them) or partitioned (g->shard_in0: the side of each ping-pong
// pair the owner partition of pag_shard_extract_range ended on) streams are now
struct StreamPtrs {
    const uint32_t *tkey;
    const uint64_t *tval;
    const uint32_t *ekey;
    const uint64_t *eval;
};
inline StreamPtrs streams_at(const pag_graph *g, int t_in0, int e_in0) {
    return StreamPtrs{(const uint32_t *)g->pool[t_in0 ? ps::TK0 : ps::TK1].p, (const uint64_t *)g->pool[t_in0 ? ps::TV0 : ps::TV1].p,
                      (const uint32_t *)g->pool[e_in0 ? ps::EK0 : ps::EK1].p, (const uint64_t *)g->pool[e_in0 ? ps::EV0 : ps::EV1].p};
}
// the tuples [t_off, +t_n) and the edges [e_off, +e_n) of the streams `x` to the starts of the four arrays, queued on s
inline int copy_streams(const StreamPtrs &x, uint64_t t_off, uint64_t t_n, uint64_t e_off, uint64_t e_n, void *tkey, void *tval, void *ekey, void *eval,
                        hipStream_t s) {
    if (t_n) PAG_HIP_TRY(hipMemcpyAsync(tkey, x.tkey + t_off, t_n * 4, hipMemcpyDeviceToDevice, s));
    if (t_n) PAG_HIP_TRY(hipMemcpyAsync(tval, x.tval + t_off, t_n * 8, hipMemcpyDeviceToDevice, s));
    if (e_n) PAG_HIP_TRY(hipMemcpyAsync(ekey, x.ekey + e_off, e_n * 4, hipMemcpyDeviceToDevice, s));
    if (e_n) PAG_HIP_TRY(hipMemcpyAsync(eval, x.eval + e_off, e_n * 8, hipMemcpyDeviceToDevice, s));
    return PAG_OK;
}

// the count lines and sizes of a graph made of parts (slices of owners, selections for a region) are the sums over the parts
inline void add_stats(pag_build_stats &st, const pag_build_stats &p) {
    for (int q = 0; q < 2; ++q) {
        st.merge_edge[q] += p.merge_edge[q];
        st.total_pos[q] += p.total_pos[q];
        st.merge_pos[q] += p.merge_pos[q];
        st.n_tuples[q] += p.n_tuples[q];
        st.n_edges[q] += p.n_edges[q];
    }
    st.n_nodes += p.n_nodes;
    st.n_pos += p.n_pos;
    st.n_uniq_edges += p.n_uniq_edges;
}
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Both extraction passes for the reads [lo, hi) of the emission order and the records per (owner, pass) of the two streams
// (pag_api.hip): pag_shard_extract_range without its partition — the streams stay as extract_stage left them, no ping-pong
// partner and no sort scratch is touched.  counts[o * 4 + q] as pag_shard_extract has them.
int shard_count_range(pag_graph *g, const pag_build_input *in, uint64_t lo, uint64_t hi, uint32_t n_shards, uint64_t *counts);

// the seven arrays of a graph (the handle's, a pag_shard_slice's) in the order of ps::GraphArr: read out, pointed elsewhere
struct GraphArrays {
    void *p[ps::GRAPH_ARRS];
};
template <typename G>
GraphArrays arrays_of(const G &x) {
    return GraphArrays{{(void *)x.tkey, (void *)x.tval, (void *)x.tseg, (void *)x.tcnt, (void *)x.ekey, (void *)x.eval, (void *)x.eseg}};
}
template <typename G>
void point_at(G &x, const GraphArrays &a) {
    x.tkey = (decltype(x.tkey))a.p[ps::G_TKEY];
    x.tval = (decltype(x.tval))a.p[ps::G_TVAL];
    x.tseg = (decltype(x.tseg))a.p[ps::G_TSEG];
    x.tcnt = (decltype(x.tcnt))a.p[ps::G_TCNT];
    x.ekey = (decltype(x.ekey))a.p[ps::G_EKEY];
    x.eval = (decltype(x.eval))a.p[ps::G_EVAL];
    x.eseg = (decltype(x.eseg))a.p[ps::G_ESEG];
}
// the arrays a family of graph slots (ps::IMPORT, ps::SEL_OUT, ps::SEND) holds now
inline GraphArrays arrays_in(const pag_graph *g, ps::Id base) {
    GraphArrays a;
    for (int i = 0; i < ps::GRAPH_ARRS; ++i) a.p[i] = g->pool[ps::family(base, i)].p;
    return a;
}

}  // namespace pagdev
