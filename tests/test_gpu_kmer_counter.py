"""GPU: the device k-mer counter (pag_kmer_count) — bit-exact against the oracle through the C ABI, the
`kmer_counter` executable byte-identical to the reference's golden files and to the reference binary on fresh reads,
and the bench-scale read set against the generator's own solid set."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmer_cases
import pagctl
import synth
from aligngraph2_amd.capi import KmerCountResult, PagSeqs
from test_kmer_counter_oracle import GOLD, oracle_file_words

EXE = os.path.join(pagctl.ROOT, "aligngraph2_amd", "bin", "kmer_counter")


def hip_count(rs, on_device, k, threshold, bitmap_ptr, bitmap_on_device):
    lib = pagctl.hip_lib()
    res = KmerCountResult()
    rc = lib.pag_kmer_count(C.byref(rs), on_device, k, threshold, 0, bitmap_ptr, bitmap_on_device, C.byref(res))
    assert rc == 0, lib.pag_last_error().decode()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("seed,k,threshold,n,hi", [(21, 3, 0.2, 50, 80), (22, 8, 0.2, 400, 900), (23, 11, 0.05, 3000, 2500),
                                                  (24, 2, 0.2, 10, 40), (25, 9, 0.0, 500, 700), (26, 10, -1.0, 100, 300),
                                                  (27, 6, 0.2, 5, 4)])
@pytest.mark.parametrize("slices", [None, "4"])  # (None: the library's own choice; "4": the table filled a quarter of the code range per launch)
def test_hip_counter_matches_oracle(seed, k, threshold, n, hi, slices, monkeypatch):
    if slices:
        monkeypatch.setenv("PAG_KC_SLICES", slices)
    case = dict(seed=seed, n=n, lo=1, hi=hi, k=k, threshold=threshold, threads=1, fmt="fastq", alphabet="ACGTNacgt")
    seqs = kmer_cases.sequences(case)
    _, mn, want = oracle_file_words(seqs, k, threshold, 1)
    offs, lens, packed = kmer_cases.pack(seqs)
    rs = PagSeqs(len(seqs), offs.ctypes.data, lens.ctypes.data, packed.ctypes.data, len(packed) - 64)
    got = np.zeros(len(want), np.uint32)
    res = hip_count(rs, 0, k, threshold, got.ctypes.data, 0)
    assert res.min_abundance == mn
    nw = (4 ** k + 31) // 32
    assert (got[:nw] == want[:nw]).all()
    assert res.n_solid == int(sum(bin(int(x)).count("1") for x in want[:nw]))
    assert res.n_kmers_counted == sum(max(0, len(s) - k + 1) for s in seqs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(kmer_cases.CASES))
def test_kmer_counter_executable_matches_golden(name, tmp_path):
    case = kmer_cases.CASES[name]
    reads = os.path.join(GOLD, name, "reads." + case["fmt"])
    out = str(tmp_path / "out.bin")
    r = subprocess.run([EXE, "-t", str(case["threads"]), "-i", reads, "-o", out, "-k", str(case["k"]), "-m", repr(case["threshold"])],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(os.path.join(GOLD, name, "expected.bin"), "rb").read()


@pytest.mark.gpu
@pytest.mark.parametrize("k,threads,fmt", [(10, 16, "fastq"), (12, 3, "fasta"), (9, 0, "fastq")])  # (-t 0: header-only file)
def test_kmer_counter_executable_matches_reference_binary(k, threads, fmt, tmp_path):
    ref = os.path.join(pagctl.REF_DIR, "kmer_counter")
    if not os.path.exists(ref):
        pytest.skip("oracle/_ref/kmer_counter was not built (needs /root/reference at build time)")
    case = dict(seed=100 + k, n=2000, lo=50, hi=3000, k=k, threshold=0.2, threads=threads, fmt=fmt, alphabet="ACGT")
    reads = str(tmp_path / ("r." + fmt))
    kmer_cases.write_reads(case, reads)
    a, b = str(tmp_path / "ours.bin"), str(tmp_path / "ref.bin")
    for exe, out in ((EXE, a), (ref, b)):
        r = subprocess.run([exe, "--thread", str(threads), "--in=" + reads, "-o" + out, "-k", str(k)], capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr
    assert open(a, "rb").read() == open(b, "rb").read()


@pytest.mark.gpu
def test_kmer_counter_usage_and_errors(tmp_path):
    assert subprocess.run([EXE], capture_output=True).returncode == 0
    assert subprocess.run([EXE, "-h"], capture_output=True).returncode == 0
    assert subprocess.run([EXE, "--nope"], capture_output=True).returncode == 1
    assert subprocess.run([EXE, "-k", "x"], capture_output=True).returncode == 1


@pytest.mark.gpu
def test_hip_counter_at_bench_scale_on_device_reads():
    """Device-resident reads of a mid-size workload: the counter reproduces the generator's histogram rule and set."""
    import torch

    import biggen
    w = biggen.BigWorkload(biggen.BigSpec(seed=5, ref_len=4_000_000, n_reads=8000, read_span=10_000, k=12), device="cuda")
    inp = w.build_input()
    nw = (4 ** 12) // 32
    bitmap = torch.zeros(nw + 8, dtype=torch.int32, device="cuda")
    res = hip_count(inp.reads, 1, 12, w.spec.solid_threshold, bitmap.data_ptr(), 1)
    torch.cuda.synchronize()
    assert res.min_abundance == w.min_abundance
    got_bits = bitmap[:nw].to(torch.int64) & 0xFFFFFFFF
    got = ((got_bits.unsqueeze(1) >> torch.arange(32, device="cuda")) & 1).bool().view(-1)
    diff = torch.nonzero(got != w.solid_mask).squeeze(1).tolist()
    assert diff in ([], [12]), diff[:10]  # code k is forced into the generator's set (file header quirk Q1)


# ---- the tail of the abundance histogram, the library's own slicing at real k, k = 15 / 16 ------------------------------

KC_TAIL = 4095  # KC_BINS - 1: abundances from here on share the histogram's last bin; the rule is then decided on the host


def _device_seqs(offs, lens, packed):
    """the reads in device memory (pag_seqs with device pointers); returns (PagSeqs, tensors to keep alive)"""
    import torch
    t = (torch.from_numpy(offs.view(np.int64)).cuda(), torch.from_numpy(lens.view(np.int32)).cuda(), torch.from_numpy(packed).cuda())
    return PagSeqs(len(lens), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(packed) - 64), t


def _count_both_residencies(seqs, k, threshold):
    """pag_kmer_count on host-resident and on device-resident reads (host bitmap): [(min_abundance, n_solid, n_kmers_counted,
    bitmap)] for each"""
    offs, lens, packed = kmer_cases.pack(seqs)
    nw = max(1, 4 ** k // 32)
    out = []
    for on_device in (0, 1):
        if on_device:
            rs, keep = _device_seqs(offs, lens, packed)
        else:
            rs = PagSeqs(len(seqs), offs.ctypes.data, lens.ctypes.data, packed.ctypes.data, len(packed) - 64)
        got = np.zeros(nw, np.uint32)
        res = hip_count(rs, on_device, k, threshold, got.ctypes.data, 0)
        out.append((res.min_abundance, res.n_solid, res.n_kmers_counted, got))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("threshold", [0.2, 0.05, 0.0])
@pytest.mark.parametrize("k", [3, 4])
def test_hip_counter_rule_decided_in_the_tail(k, threshold):
    """~1.5 Mbases over 4^k <= 256 codes: every abundance is >= 4095, so the minimum abundance comes from the exact tail the
    host reads back from the table — against the oracle, on host- and device-resident reads."""
    case = dict(seed=60 + k, n=300, lo=4000, hi=6000, k=k, threshold=threshold, alphabet="ACGTN")
    seqs = kmer_cases.sequences(case)
    _, mn, want = oracle_file_words(seqs, k, threshold, 1)
    assert mn >= KC_TAIL, mn
    nw = 4 ** k // 32
    n_kmers = sum(max(0, len(s) - k + 1) for s in seqs)
    for on_device, (got_mn, n_solid, n_counted, got) in enumerate(_count_both_residencies(seqs, k, threshold)):
        assert got_mn == mn, (on_device, got_mn, mn)
        assert (got[:nw] == want[:nw]).all(), on_device
        assert n_solid == int(np.unpackbits(want[:nw].view(np.uint8)).sum()), on_device
        assert n_counted == n_kmers, (on_device, n_counted, n_kmers)
    print(f"k={k} threshold={threshold}: min_abundance {mn}")


@pytest.mark.gpu
@pytest.mark.parametrize("threshold", [0.2, 0.5])
def test_hip_counter_tail_present_rule_stops_before_it(threshold):
    """A-rich reads: AAAA's abundance reaches the last bin, the rule stops far below it (and the k-mers counted stay exact)."""
    k = 4
    case = dict(seed=70, n=40, lo=4000, hi=6000, k=k, threshold=threshold, alphabet="AAAAAAACGT")
    seqs = kmer_cases.sequences(case)
    _, mn, want = oracle_file_words(seqs, k, threshold, 1)
    codes = np.concatenate([synth.kmer_codes(np.frombuffer(s.encode(), np.uint8), k) for s in seqs])
    assert np.bincount(codes.astype(np.int64), minlength=4 ** k).max() >= KC_TAIL
    assert 0 < mn < KC_TAIL, mn
    nw = 4 ** k // 32
    for on_device, (got_mn, n_solid, n_counted, got) in enumerate(_count_both_residencies(seqs, k, threshold)):
        assert got_mn == mn, (on_device, got_mn, mn)
        assert (got[:nw] == want[:nw]).all(), on_device
        assert n_solid == int(np.unpackbits(want[:nw].view(np.uint8)).sum()), on_device
        assert n_counted == len(codes), (on_device, n_counted, len(codes))


# reads for the large-k cases: forward-strand fragments of a 60 kb genome at ~5x (abundances of a few), some with N, lengths
# at the 1024-position tiles' edges (k-mer start counts 1023 .. 1025, = 0 / 1 / 15 mod 16) and shorter than k
def _genome_reads(seed, k):
    rng = np.random.default_rng(seed)
    genome = synth.random_seq(rng, 60_000)
    lens = [n + k - 1 for n in (1023, 1024, 1025, 1008, 1009, 1039, 2048, 2049, 2063, 17, 16, 15, 1)] + [k - 1, 3]
    total = sum(lens)
    while total < 300_000:
        lens.append(int(rng.integers(200, 6000)))
        total += lens[-1]
    seqs = []
    for L in lens:
        s = int(rng.integers(0, len(genome) - L))
        r = genome[s:s + L].copy()
        r[rng.random(L) < 0.002] = ord("N")
        seqs.append(r.tobytes().decode())
    return seqs


def _numpy_rule(seqs, k):
    """the reference's rule over np.unique of the forward-strand codes (non-ACGT -> A): a threshold half-way between two
    steps of the cumulative histogram, chosen so that the rule stops at abundance 3, and the solid codes {abundance >= 3}"""
    codes = np.concatenate([synth.kmer_codes(np.frombuffer(s.encode(), np.uint8), k) for s in seqs])
    uniq, cnt = np.unique(codes, return_counts=True)
    n = 4 ** k
    vals, nvals = np.unique(cnt, return_counts=True)
    hist = [(0, n - len(uniq))] + list(zip(vals.tolist(), nvals.tolist()))
    above = {a: int((cnt > a).sum()) for a, _ in hist}  # codes with abundance > a
    assert 2 in above and 3 in above
    threshold = (above[2] + above[3]) / 2 / n
    mn, s = 0, 0
    for a, h in hist:  # kmer_counter.cpp:59-77, in double
        s += h
        if 1 - s * 1.0 / n <= threshold:
            mn = a
            break
    assert mn == 3
    return threshold, mn, uniq[cnt >= mn], len(codes)


@pytest.mark.gpu
@pytest.mark.parametrize("k,resident", [(13, "host"), (14, "host"), (14, "device"), (15, "device"), (16, "device")])
def test_hip_counter_default_slicing_at_large_k(k, resident, monkeypatch):
    """k >= 13: the library fills the table a slice of the code range per launch of its own accord (no PAG_KC_SLICES);
    k = 15 / 16: tables of 4 / 16 GB.  Against a numpy reference; the device bitmap is compared through its non-zero words."""
    import torch
    monkeypatch.delenv("PAG_KC_SLICES", raising=False)
    seqs = _genome_reads(80 + k, k)
    threshold, mn, want_codes, n_kmers = _numpy_rule(seqs, k)
    offs, lens, packed = kmer_cases.pack(seqs)
    if resident == "device":
        rs, keep = _device_seqs(offs, lens, packed)
    else:
        rs = PagSeqs(len(seqs), offs.ctypes.data, lens.ctypes.data, packed.ctypes.data, len(packed) - 64)
    nw = 4 ** k // 32
    bitmap = torch.zeros(nw, dtype=torch.int32, device="cuda")
    res = hip_count(rs, 1 if resident == "device" else 0, k, threshold, bitmap.data_ptr(), 1)
    torch.cuda.synchronize()
    assert res.min_abundance == mn
    assert res.n_kmers_counted == n_kmers
    assert res.n_solid == len(want_codes)
    widx = torch.nonzero(bitmap).squeeze(1)
    words = bitmap[widx].cpu().numpy().view(np.uint32)
    widx = widx.cpu().numpy().astype(np.uint64)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little").reshape(-1, 32).astype(bool)
    got_codes = (widx[:, None] * np.uint64(32) + np.arange(32, dtype=np.uint64)[None, :])[bits]
    assert len(got_codes) == len(want_codes) and (np.sort(got_codes) == want_codes).all()
    del bitmap
    torch.cuda.empty_cache()
