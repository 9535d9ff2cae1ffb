"""CPU: every case of tests/prep_cases.py still reaches the path it was made for — read off the host restatement's arrays
(LoadedInput.view), the parser's records (raw_view) and the C oracle.  The GPU tests that run these cases
(test_gpu_prepare.py) rely on what is asserted here."""
import numpy as np
import pytest

import pagctl
import prep_cases
from aligngraph2_amd.workload import FLAG_ELIG, PAG_NONE

TOPKS = ((0, 0), (1, 1), (2, 1), (1, 16), (-1, 3))  # (topk_ctg, topk_ref) of test_gpu_prepare.py's topk test

_loaded = {}


@pytest.fixture(scope="module")
def cases(workdir):
    for name in prep_cases.CASES:
        d, case = prep_cases.generate(name, str(workdir / ("prep_cases_cpu_" + name)))
        inp = pagctl.LoadedInput(d, threads=case.threads, eps=case.eps, cov=case.cov)
        _loaded[name] = (inp, case, prep_cases.host_view(inp), prep_cases.raw_records(inp))
    yield _loaded
    for inp, *_ in _loaded.values():
        inp.close()
    _loaded.clear()


def _raw_lists(raw, n_reads):
    """per read: database indices of its records with both names known, database order (what mergeAlignInfHelper collects)"""
    listed = np.flatnonzero((raw["query"] != PAG_NONE) & (raw["target"] != PAG_NONE))
    return [listed[raw["query"][listed] == r] for r in range(n_reads)]


@pytest.mark.parametrize("name", ["list_lengths", "reject"])
def test_list_lengths_reach_the_insertion_sort_and_the_fast_counts_switch(name, cases):
    inp, case, v, (raw1, raw2) = cases[name]
    for which, raw, aln, qoff in (("read->contig", raw1, v["aln1"], v["qoff1"]), ("read->reference", raw2, v["aln2"], v["qoff2"])):
        kept = np.diff(qoff.astype(np.int64))
        if name == "list_lengths":
            assert set(range(2, 19)) <= set(kept.tolist()), f"{which}: kept list lengths {sorted(set(kept.tolist()))}"
        assert {15, 16, 17} <= set(kept.tolist()) or name == "reject" and (kept == 16).any() and (kept > 16).any()
        # the lists pag_prepare sorts (before the static filters): 16 = the longest the device's insertion sort takes, 17 = the
        # shortest that goes to the host's std::sort; each with a tie between entries that are not neighbours in the database
        lists = _raw_lists(raw, v["n_reads"])
        assert any(3 <= len(l) <= 15 for l in lists) and any(len(l) == 16 for l in lists) and any(len(l) > 16 for l in lists)
        for n in (16, 17) if name == "list_lengths" else ():
            found = False
            for l in lists:
                if len(l) != n:
                    continue
                sc = raw["score"][l]
                for s in np.unique(sc):
                    idx = l[sc == s]
                    if len(idx) >= 2 and (np.diff(idx) > 1).any():
                        found = True
            assert found, f"{which}: no list of {n} with a tie between records apart in the database"
    # K1's fast_counts switch (n_act <= 15, k1_extract.hip): read strands with exactly 15 and exactly 16 active alignments, in both
    # passes; no contig has multi-entry bases, so in pass 1 that count alone decides
    assert not v["ctgs"]["multi"].any()
    for aln, qoff in ((v["aln1"], v["qoff1"]), (v["aln2"], v["qoff2"])):
        act = prep_cases.active_per_strand(aln, qoff, v["n_reads"])
        assert (act == 15).any() and (act == 16).any(), sorted(set(act.ravel().tolist()))


@pytest.mark.parametrize("name", ["cov_only", "reject"])
def test_coverage_only_records_exist_from_both_causes_and_decide(name, cases):
    inp, case, v, (_, raw2) = cases[name]
    a2 = v["aln2"]
    n_listed = int(v["qoff2"][-1])
    assert (a2["query"][:n_listed] != PAG_NONE).all() and (a2["query"][n_listed:] == PAG_NONE).all()
    assert (a2["query"] == PAG_NONE).sum() > 0
    # cause 1: the read's name is unknown; cause 2: a known read, the accepted reference, the query interval below 0.10 of the read
    accepted = int(np.flatnonzero(v["refs"]["accepted"])[0])
    unknown = (raw2["query"] == PAG_NONE) & (raw2["target"] == accepted)
    known = (raw2["query"] != PAG_NONE) & (raw2["target"] == accepted)
    ratio = np.zeros(len(raw2))
    ratio[known] = (raw2["q_end"][known] - raw2["q_begin"][known]).astype(np.float64) / v["read_len"][raw2["query"][known]]
    short = known & (ratio < 0.10)
    assert unknown.sum() > 0 and short.sum() > 0
    assert (a2["query"] == PAG_NONE).sum() >= unknown.sum() + short.sum()
    # they decide: without them some listed record's verdict at the case's cov is another
    full, _ = prep_cases.numpy_cov_verdicts(a2, v["refs"], case.cov)
    part, _ = prep_cases.numpy_cov_verdicts(a2[:n_listed], v["refs"], case.cov)
    assert (full[:n_listed] != part).sum() >= 5
    assert 0 < full[:n_listed].sum() < n_listed


@pytest.mark.parametrize("name", ["other_ref", "reject"])
def test_records_on_other_targets_exist_and_are_clamped(name, cases):
    inp, case, v, (raw1, raw2) = cases[name]
    a2 = v["aln2"]
    refs = v["refs"]
    assert len(refs) == 3 and refs["accepted"].tolist() == [1, 0, 0]
    tail = a2[a2["query"] == PAG_NONE]
    other = tail[refs["accepted"][tail["target"]] == 0]
    assert len(other) > 0
    assert (other["t_end"] <= refs["len"][other["target"]]).all() and (other["t_begin"] <= other["t_end"]).all()
    assert ((other["t_end"] == refs["len"][other["target"]]) & (other["t_begin"] < other["t_end"])).any(), "no interval clamped to a decoy's end"
    assert ((other["t_begin"] == other["t_end"]) & (other["t_end"] == refs["len"][other["target"]])).any(), "no interval wholly past a decoy's end"
    assert (raw2["t_end"][raw2["target"] != PAG_NONE] > refs["len"][raw2["target"][raw2["target"] != PAG_NONE]]).any()
    # the listed records are all on the accepted reference
    listed = a2[a2["query"] != PAG_NONE]
    assert (refs["accepted"][listed["target"]] == 1).all()
    # read->contig: a target that is no contig, and (other_ref) a contig the block does not list
    assert ((raw1["query"] != PAG_NONE) & (raw1["target"] == PAG_NONE)).any()
    if case.unlisted_ctg:
        sel = v["ctgs"]["selected"]
        assert sel.tolist() == [1, 1, 0]
        assert (sel[raw1["target"][raw1["target"] != PAG_NONE]] == 0).any()
        assert (sel[v["aln1"]["target"]] == 1).all()


def test_reject_cov_rejects_part_of_pass_two_and_topk_meets_rejected_alignments(cases):
    inp, case, v, _ = cases["reject"]
    tuples = {}
    try:
        for cov in (0, case.cov, 100000):
            inp.set_cov(cov)
            tuples[cov] = int(pagctl.run_oracle(inp)["stats"].n_tuples[1])
    finally:
        inp.set_cov(case.cov)
    print("pass-2 tuples by cov:", tuples)
    assert tuples[100000] == 0
    assert 0.10 * tuples[0] <= tuples[case.cov] <= 0.90 * tuples[0], tuples
    # topk: for some read the first topk_ref LISTED alignments are not the first topk_ref that PASS the filter, so that it matters
    # that for_active (k1_extract.hip) does not count rejected alignments (Aligner.tcc:121-123, 147, 166)
    a2, qoff = v["aln2"], v["qoff2"].astype(np.int64)
    ok, _ = prep_cases.numpy_cov_verdicts(a2, v["refs"], case.cov)
    for topk in sorted({t for _, t in TOPKS if t > 0}):
        differ = 0
        for r in range(v["n_reads"]):
            idx = np.arange(qoff[r], qoff[r + 1])
            idx = idx[(a2["flags"][idx] & FLAG_ELIG) != 0]
            # counting the rejected ones too would leave this read fewer alignments than it gets
            differ += int(ok[idx[:topk]].sum()) < min(topk, int(ok[idx].sum()))
        print(f"topk_ref {topk}: {differ} reads whose first {topk} listed alignments are not the first {topk} that pass")
        assert differ > 0, f"topk_ref {topk}: rejected alignments never stand in front of accepted ones"
    # ... and the oracle's result depends on topk at all
    try:
        inp.set_topk(1, 1)
        cut = int(pagctl.run_oracle(inp)["stats"].n_tuples[1])
    finally:
        inp.set_topk(-1, -1)
    assert 0 < cut < tuples[case.cov]
