// cns_rows.hpp — the rows pa_cns's graphs are built from, as plain functions over byte pointers: one part's slice of an alignment
// (AlignData::sliceHelper, tools/cns/AlignData.cpp:11-34) and dagcon's gap normalisation of it (normalizeGaps(aln, push = true),
// tools/cns/Alignment.cpp:131-217).  One source, compiled for the device (csrc/hip/k_cns_rows.hip: a slice per lane) and for host
// threads (bin/pa_cns, PA_CNS_INGEST=flat; the library's oversize path) — the way cns_graph.hpp is.  No std::string, no
// allocation: the caller owns every buffer, every loop is bounded by the slice's column count.
//
// Bytes are compared as bytes: lower case, 'N' and '\r' are ordinary symbols; '.' is a gap for normalize_gaps (its first pass)
// and an ordinary symbol for slice_bounds, as in the reference.
#pragma once
#include <stdint.h>

#ifndef CNS_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CNS_HD __host__ __device__ inline
#else
#define CNS_HD inline
#endif
#endif

namespace pagrows {

// one slice to cut and normalise (= pag_cns_slice, include/pagraph_hip.h)
struct Slice {
    uint64_t q_off, t_off;    // the record's two rows in the text
    uint64_t origin_start;    // backbone position of the record's first target base (refBegin)
    uint64_t slice_start, slice_end;  // the part's backbone interval
    uint64_t out_off;         // its slot in the two pools: [out_off, out_off + out_cap)
    uint32_t n_cols;          // columns of the record
    uint32_t out_cap;         // >= 2 x the slice's columns (every column can become two)
    uint32_t slot;            // where its result goes in the caller's array
    uint32_t reserved;
};
// what came out (= pag_cns_row)
struct Row {
    uint64_t str_off;         // = out_off
    uint32_t len;             // columns after normalisation (the slice's columns before it when flag != 0)
    uint32_t n_ins;           // columns with a query symbol over a target gap: the nodes the part's graph gains
    uint32_t n_edge_cols;     // columns whose query is not a gap: the edges it may gain
    uint32_t flag;            // ROW_*
};
enum { ROW_OK = 0, ROW_OVERSIZE = 1 /* more columns than the work rows hold: not done */, ROW_E_SLOT = 2 /* out_cap < 2 x columns */ };

// The [left, right) columns of the target row `t` (n_cols columns, first base at backbone position origin_start) that belong to
// the backbone interval [slice_start, slice_end).  Only '-' is a gap.  Gap columns at the very start of a record are skipped;
// gap columns just before a part boundary belong to the earlier slice; trailing gap columns belong to the last one.
CNS_HD void slice_bounds(const char *t, uint32_t n_cols, uint64_t origin_start, uint64_t slice_start, uint64_t slice_end, uint32_t *left, uint32_t *right) {
    uint32_t l, r;
    uint64_t cnt = 0;
    for (l = 0; l < n_cols; ++l) {
        if (t[l] == '-') continue;
        if (origin_start + cnt >= slice_start) break;
        ++cnt;
    }
    for (r = l; r < n_cols; ++r) {
        if (t[r] == '-') continue;
        if (origin_start + cnt >= slice_end) break;
        ++cnt;
    }
    *left = l;
    *right = r;
}

struct Counts {
    uint32_t len, n_ins, n_edge_cols;
};

// q, t: n columns.  wq, wt: work rows of at least 2 n columns, column i at [i * ws] (ws = 1: a plain row; the device keeps the
// 64 rows of a wavefront column by column, ws = 64).  qo, to: the normalised rows, at most 2 n columns; they may be the work
// rows themselves when ws = 1 (the last pass writes behind its reads).
CNS_HD Counts normalize_gaps(const char *q, const char *t, uint32_t n, char *wq, char *wt, uint32_t ws, char *qo, char *to) {
    // dots to dashes, mismatches to indels: a mismatch column becomes -/q after t/-
    uint64_t m = 0;
    for (uint32_t i = 0; i < n; ++i) {
        char qb = q[i], tb = t[i];
        if (qb == '.') qb = '-';
        if (tb == '.') tb = '-';
        if (qb != tb && qb != '-' && tb != '-') {
            wq[m * ws] = '-';
            wt[m * ws] = tb;
            ++m;
            wq[m * ws] = qb;
            wt[m * ws] = '-';
            ++m;
        } else {
            wq[m * ws] = qb;
            wt[m * ws] = tb;
            ++m;
        }
    }
    // push gaps to the right, but not past the end: a chain of dependent accesses, column after column
    for (uint64_t i = 0; i + 1 < m; ++i) {
        if (wt[i * ws] == '-') {
            uint64_t j = i;
            while (++j < m) {
                const char c = wt[j * ws];
                if (c != '-') {
                    if (c == wq[i * ws]) {
                        wt[i * ws] = c;
                        wt[j * ws] = '-';
                    }
                    break;
                }
            }
        }
        if (wq[i * ws] == '-') {
            uint64_t j = i;
            while (++j < m) {
                const char c = wq[j * ws];
                if (c != '-') {
                    if (c == wt[i * ws]) {
                        wq[i * ws] = c;
                        wq[j * ws] = '-';
                    }
                    break;
                }
            }
        }
    }
    // columns of two gaps are dropped; the counts that size the part's graph
    Counts c{0, 0, 0};
    for (uint64_t i = 0; i < m; ++i) {
        const char qb = wq[i * ws], tb = wt[i * ws];
        if (qb != '-' || tb != '-') {
            qo[c.len] = qb;
            to[c.len] = tb;
            ++c.len;
            if (qb != '-') {
                ++c.n_edge_cols;
                if (tb == '-') ++c.n_ins;
            }
        }
    }
    return c;
}

// One slice from the text to its slot in the pools.  wq == nullptr: the slot itself is the work space (host threads);
// otherwise work rows of `stage_cols` columns with stride ws, and a slice that may outgrow them is flagged, not done.
CNS_HD Row run_slice(const char *text, const Slice &S, char *wq, char *wt, uint32_t ws, uint32_t stage_cols, char *qpool, char *tpool) {
    uint32_t l, r;
    slice_bounds(text + S.t_off, S.n_cols, S.origin_start, S.slice_start, S.slice_end, &l, &r);
    const uint32_t n = r - l;
    Row R{S.out_off, n, 0, 0, ROW_OK};
    if (2ull * n > S.out_cap) {
        R.flag = ROW_E_SLOT;
        return R;
    }
    char *qo = qpool + S.out_off, *to = tpool + S.out_off;
    if (!wq) {
        wq = qo;
        wt = to;
        ws = 1;
    } else if (2ull * n > stage_cols) {
        R.flag = ROW_OVERSIZE;
        return R;
    }
    const Counts c = normalize_gaps(text + S.q_off + l, text + S.t_off + l, n, wq, wt, ws, qo, to);
    R.len = c.len;
    R.n_ins = c.n_ins;
    R.n_edge_cols = c.n_edge_cols;
    return R;
}

}  // namespace pagrows
