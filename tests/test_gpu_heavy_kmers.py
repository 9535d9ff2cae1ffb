"""GPU parity of the graph build on heavy k-mers: single segments of 150 000 records (one wavefront each in K3 and K4), a u16 count
that wraps, dozens of k-mers on cluster_long's in-place path and edges_long's through-memory path in one build.  HIP library vs the
C oracle, which tests/test_oracle_graph_only.py and test_oracle_golden.py pin to the compiled reference."""
import time

import numpy as np
import pytest

import heavy_cases
import pagctl
import synth

# pag_process on an MI355X, measured once per case: 29.4 s (count_wrap_t8), 28.2 s (eps 5) and 29.4 s (eps 1), nearly all of it one
# wavefront of edges_long rank-sorting the poly-A k-mer's 150 000 edge records through memory (quadratic: about 80 ns per inner step;
# the same kernel needs 13 s for 100 000 records and 50 s for 200 000 in tests/harness/seg_kernels_test).  A finding about the product —
# a real genome's poly-A k-mer goes the same way — that these tests record and do not fix.  They fail when a build takes ten times as long.
WRAP_LIMIT_S = 10 * 29.4
MANY_LIMIT_S = 10 * 29.4


def _build_both_ways(inp, ora, label, limit_s):
    for prepare in (True, False):  # device-prepared input (the product path), host-prepared input
        t0 = time.time()
        hip = pagctl.run_hip(inp, streams=True, prepare=prepare)
        wall = time.time() - t0
        st = hip["stats"]
        print(f"{label} prepare={prepare}: run_hip {wall:.2f} s, pag_process {st.ms_total / 1e3:.2f} s")
        pagctl.compare_results(hip, ora, label=f"{label} prepare={prepare}")
        assert st.ms_total / 1e3 < limit_s, f"{label}: pag_process took {st.ms_total / 1e3:.1f} s"


@pytest.mark.gpu
def test_count_wrap_build_matches_oracle(workdir):
    """tests/golden/graph_only/count_wrap_t8: streams, count lines and every CSR array (pos_cnt with its wrapped count).  Build only.
    pag_process on an MI355X: 29.4 s with the device-prepared input, 28.8 s with the host-prepared one."""
    name = "count_wrap_t8"
    spec, golden = heavy_cases.load(name)
    ind = heavy_cases.materialize(name, str(workdir / name))
    inp = pagctl.LoadedInput(ind, threads=spec["threads"], eps=spec["epsilon"], cov=spec["cov"])
    try:
        ora = pagctl.run_oracle(inp, streams=True)
        deficits = heavy_cases.count_deficits(ora)
        assert deficits and all(raw > s and (raw - s) % 65536 == 0 for _, raw, s in deficits), deficits
        assert list(ora["stats"].counts()) == golden["counts"]
        _build_both_ways(inp, ora, name, WRAP_LIMIT_S)
    finally:
        inp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("eps", [5, 1])
def test_many_long_segments_build_matches_oracle(eps, workdir):
    """heavy_cases.MANY_LEADERS: by the oracle's arrays at least 20 k-mers with more than 512 leaders (measured: 28, the most 2 248 at
    eps 5 and 5 928 at eps 1) and at least 20 with more than 1 024 raw edges (28, the most 147 511).  pag_process on an MI355X:
    28.2 / 28.0 s at eps 5 and 29.4 / 28.9 s at eps 1 (device-prepared / host-prepared input)."""
    kw, threads, _, cov = heavy_cases.MANY_LEADERS
    d = str(workdir / f"many_leaders_eps{eps}")
    synth.generate(synth.Spec(**kw), d)
    inp = pagctl.LoadedInput(d, threads=threads, eps=eps, cov=cov)
    try:
        ora = pagctl.run_oracle(inp, streams=True)
        leaders, raw_edges = heavy_cases.leaders_and_raw_edges(ora)
        assert int((leaders > 512).sum()) >= 20 and int((raw_edges > 1024).sum()) >= 20, (leaders.max(), raw_edges.max())
        _build_both_ways(inp, ora, f"many_leaders_eps{eps}", MANY_LIMIT_S)
    finally:
        inp.close()
