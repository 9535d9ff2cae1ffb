"""Graph builds with heavy k-mers (a poly-A tract under long reads): the inputs of tests/golden/graph_only/ and of
test_gpu_heavy_kmers.py, and what the tests read off a result about them."""
import hashlib
import json
import os

import numpy as np

import goldens
import synth

GRAPH_ONLY = os.path.join(goldens.GOLDEN, "graph_only")

# The family of the count_wrap_t8 golden at three times the length and an epsilon of 5: the poly-A k-mers keep thousands of leaders
# (cluster_long's in-place path) and hold up to 150 000 raw edges (edges_long's rank sort through memory).  (Spec kwargs, threads, eps, cov)
MANY_LEADERS = (dict(seed=131, ref_len=30000, n_reads=300, read_len=6000, k=9, solid_min_abundance=2,
                     contigs=[(200, 14000, False), (15000, 29800, False)], homopolymer=(3000, 8000)), 8, 5, 2)


def load(name):
    case = os.path.join(GRAPH_ONLY, name)
    return json.load(open(os.path.join(case, "spec.json"))), json.load(open(os.path.join(case, "graph.json")))


def materialize(name, dest):
    """the inputs of a graph-only golden, generated from its spec (and rewritten, where the spec names rewrites of
    tests/prep_cases.py) and checked against the committed hashes"""
    spec, _ = load(name)
    goldens.generate_case(spec, dest)
    if spec.get("rewrite"):
        import prep_cases
        prep_cases.apply_rewrites(dest, spec["rewrite"], spec.get("unlisted_ctg", ""))
    want = json.load(open(os.path.join(GRAPH_ONLY, name, "inputs.sha256")))
    assert sorted(os.listdir(dest)) == sorted(want), f"{name}: input files {sorted(os.listdir(dest))}"
    for f, h in want.items():
        got = hashlib.sha256(open(os.path.join(dest, f), "rb").read()).hexdigest()
        assert got == h, f"golden input drift in graph_only/{name}/{f}"
    return dest


def count_deficits(res):
    """nodes of a pagctl result (streams kept) whose u16 counts do not sum to their raw tuples: [(code, raw tuples, count sum)]"""
    csr = res["csr"]
    codes, raw = np.unique(res["streams"]["tkey"], return_counts=True)
    assert np.array_equal(codes, csr["node_code"])
    sums = np.add.reduceat(csr["pos_cnt"].astype(np.uint64), csr["pos_off"][:-1].astype(np.int64))
    return [(int(codes[i]), int(raw[i]), int(sums[i])) for i in np.flatnonzero(sums != raw.astype(np.uint64))]


def leaders_and_raw_edges(res):
    """per k-mer of a pagctl result (streams kept): clustered positions (= leaders of its tuple segment), raw edge records"""
    leaders = np.diff(res["csr"]["pos_off"].astype(np.int64))
    _, raw_edges = np.unique(res["streams"]["ekey"], return_counts=True)
    return leaders, raw_edges
