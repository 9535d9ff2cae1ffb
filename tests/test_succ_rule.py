"""CPU: tests/succ_rule.py — PABruijnGraph::successors restated in numpy over graph.txt.gz — against the compiled reference's own
dump of every vertex's successors (tests/golden/<case>/succ.txt.gz: deviation 2 * epsilon, error rate 0.15), record for record.
The restatement is what tests/test_gpu_succ_query.py holds pag_successors_batch to at the parameters no golden covers."""
import numpy as np
import pytest

import goldens
import succ_rule


@pytest.mark.parametrize("name", ["extend_gap_t1", "eps20_k11_jitter_t16", "succ_corners_t8"])
def test_the_restatement_gives_the_reference_s_lists(name):
    eps = goldens.load_spec(name)["epsilon"]
    graphs, dumps = succ_rule.load_graph(name), succ_rule.reference_dump(name)
    assert len(graphs) == len(dumps)
    for g, d in zip(graphs, dumps):
        v = succ_rule.vertex_ids(g, d["key"][:, 0], d["key"][:, 1])
        assert np.array_equal(np.sort(v), np.arange(len(g["ctg"]))), "the dump lists every vertex of the graph once"
        off, rec = succ_rule.successors(g, v, 2 * eps, 0.15)
        want = np.concatenate((succ_rule.vertex_ids(g, d["rec"][:, 0], d["rec"][:, 1])[:, None], d["rec"][:, 2:]), axis=1)
        differing = np.flatnonzero(np.diff(off) != np.diff(d["off"]))
        assert len(differing) == 0, f"{name}: {len(differing)} vertices with another list length, first {d['key'][differing[0]].tolist()}"
        assert np.array_equal(rec, want), f"{name}: first differing record {int(np.flatnonzero((rec != want).any(axis=1))[0])}"


def test_check_position_corners():
    """the quirks the vectorised form must keep: wrap-around differences, a step of 0, the un-guarded second ratio test"""
    u = lambda *x: np.array(x, dtype=np.uint32)  # noqa: E731
    # parent (100, 0) -> child (110, 0), step 10: contig side exact; no reference coordinate on either side -> Good
    g, e = succ_rule.check_position(u(100), u(0), u(110), u(0), u(10), 20, 0.15)
    assert (g[0], e[0]) == (succ_rule.GOOD, True)
    # a child BEHIND its parent: the u32 difference wraps to ~4e9, no ratio holds, but |(100 + 10) - 95| <= 20 does
    g, e = succ_rule.check_position(u(100), u(0), u(95), u(0), u(10), 20, 0.15)
    assert (g[0], e[0]) == (succ_rule.GOOD, True)
    g, e = succ_rule.check_position(u(100), u(0), u(95), u(0), u(10), 0, 0.15)
    assert (g[0], e[0]) == (succ_rule.OOPS, False)
    # step 0: the ratio divides by zero and never holds; the deviation alone decides
    g, e = succ_rule.check_position(u(100), u(7), u(100), u(7), u(0), 0, 0.15)
    assert (g[0], e[0]) == (succ_rule.AMAZING, True)
    # un-guarded ratio (checkPosition :155-156): parent without a contig coordinate, child at ctg = step: the ratio "0 -> 10 over
    # 10" holds although isEdgeSimilar().first is false; the reference side fails -> the first case returns Oops all the same
    g, e = succ_rule.check_position(u(0), u(50), u(10), u(500), u(10), 20, 0.15)
    assert (g[0], e[0]) == (succ_rule.OOPS, False)
    # ... and where the reference side holds (exactly: deviation 0, error rate 0) a child WITH a contig coordinate is Excellent
    g, e = succ_rule.check_position(u(0), u(50), u(10), u(60), u(10), 0, 0.0)
    assert (g[0], e[0]) == (succ_rule.EXCELLENT, False)
