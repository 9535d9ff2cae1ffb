"""GPU: K1 (csrc/hip/k1_extract.hip) at the parameters the pipeline's defaults never reach — HIP build vs the C oracle,
bit-exact: emitted tuple / edge streams, count lines, every CSR array (pagctl.compare_results).

- outer_sample 1..7 (pag_build_input.outer_sample; the C ABI accepts 1..7).  The kernel has three builds: S <= 3 runs the
  sampler as byte tables composed by one byte permute, S = 4..7 as nibble tables, and S < 3 takes the MAXS = 1024 LDS
  build, whose emit phase needs more than one turn once a tile keeps more than 384 samples.  Both input paths: the
  device-prepared input (pag_prepare, outer_sample set in the raw input) and the host-prepared one; the oracle
  (oracle/pag_oracle.c, sampleSequence for any outer_sample) gets the same value through the host view.
- read lengths at tile edges: k-mer start counts 1023 / 1024 / 1025 and values = 0, 1, 15 (mod 16), reads shorter than k.
- a complete solid set (every code solid: K1 skips the solid-mask gather) made by pag_create and by pag_create_from_bitmap.
- rejected outer_sample values, and a valid build on the same handle afterwards.

outer_sample != 3 has no counterpart in the compiled reference (its pagraph.cpp hard-codes 3): the oracle is the reference
here.
"""
import ctypes as C

import numpy as np
import pytest

import pagctl
import synth

PAG_EINVAL = -22
K = 10
# k-mer start positions per read strand: both sides of the 1024-position tile, = 0 / 1 / 15 (mod 16), tiny; then two reads
# shorter than k (one of k - 1 bases, one of 4)
EDGE_NPOS = (1023, 1024, 1025, 1008, 1009, 1039, 2048, 2049, 2063, 17, 16, 15, 1)
EDGE_LENS = tuple(n + K - 1 for n in EDGE_NPOS) + (K - 1, 4)

CASES = {
    # name: (Spec kwargs, threads).  dense: every read k-mer solid, no clipping, reads of ~3 500 bases (several tiles per
    # strand) — at outer 1 whole tiles are kept (the emit loop's later turns).  sparse: solid = abundance >= 2, planted
    # repeats, a reverse contig, multi-entry contig bases, duplicate alignments — candidate gaps of every size.
    "dense": (dict(seed=31, ref_len=20000, n_reads=40, read_len=3500, read_len_jitter=0.2, k=K, clip_frac=0.0, solid_min_abundance=1,
                   contigs=[(100, 9800, False), (10100, 19800, True)], read_lens=EDGE_LENS), 1),
    "sparse": (dict(seed=32, ref_len=24000, n_reads=160, read_len=1500, read_len_jitter=0.6, k=K, solid_min_abundance=2, repeats=3,
                    contigs=[(200, 11000, False), (11300, 23600, True)], extra_ctg_aln=True, dup_read_aln=True, read_lens=EDGE_LENS), 4),
}

_inputs = {}
_oracle = {}


@pytest.fixture(scope="module")
def inputs(workdir):
    for name, (kw, threads) in CASES.items():
        d = str(workdir / ("extract_params_" + name))
        synth.generate(synth.Spec(**kw), d)
        _inputs[name] = pagctl.LoadedInput(d, threads=threads)
    yield _inputs
    for inp in _inputs.values():
        inp.close()
    _inputs.clear()
    _oracle.clear()


def oracle(inp, name, outer):
    if (name, outer) not in _oracle:
        inp.set_outer_sample(outer)
        _oracle[(name, outer)] = pagctl.run_oracle(inp, streams=True)
    return _oracle[(name, outer)]


def test_read_lengths_at_tile_edges():
    """synth's read_lens gives the reads exactly these lengths (what the cases above rely on)"""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        synth.generate(synth.Spec(seed=3, ref_len=8000, n_reads=len(EDGE_LENS) + 3, read_len=600, k=K, read_lens=EDGE_LENS), d)
        seqs = open(d + "/0.new.fastq").read().split("\n")[1::4]
    assert tuple(len(s) for s in seqs[:len(EDGE_LENS)]) == EDGE_LENS
    assert {len(s) - K + 1 for s in seqs} >= {1023, 1024, 1025}


@pytest.mark.gpu
@pytest.mark.parametrize("prepare", [True, False], ids=["device_prepared", "host_prepared"])
@pytest.mark.parametrize("outer", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("name", list(CASES))
def test_extract_outer_sample_matches_oracle(name, outer, prepare, inputs):
    inp = inputs[name]
    ora = oracle(inp, name, outer)
    inp.set_outer_sample(outer)
    hip = pagctl.run_hip(inp, streams=True, prepare=prepare)
    pagctl.compare_results(hip, ora, label=f"{name} outer={outer} prepare={prepare}")
    assert hip["stats"].n_pos > 0 and len(ora["streams"]["ekey"]) > 0
    # coverage of the paths named in the docstring, derived from the oracle so that it cannot silently go away
    if name == "dense" and outer == 1:
        assert ora["max_tile_samples"] > 384, ora["max_tile_samples"]  # (MAXS = 1024 build: emit phase beyond one turn)
    if name == "sparse" and outer == 1:  # every candidate kept: the edge steps are the candidate gaps
        steps = set(((ora["streams"]["eval"] >> np.uint64(1)) & np.uint64(0x7FFFFFFF)).tolist())
        assert set(range(1, 9)) <= steps, sorted(steps)[:12]


@pytest.mark.gpu
@pytest.mark.parametrize("outer", [1, 3, 5])
@pytest.mark.parametrize("how", ["codes", "bitmap"])
def test_extract_complete_solid_set(how, outer, workdir):
    """Every one of the 4^k codes solid (k = 5): the handle reports all_solid and K1 skips the solid-mask gather."""
    k = 5
    d = str(workdir / "extract_all_solid")
    synth.generate(synth.Spec(seed=41, ref_len=9000, n_reads=50, read_len=900, read_len_jitter=0.5, k=k,
                              contigs=[(100, 4300, False), (4600, 8800, True)], read_lens=(1023 + k - 1, 1025 + k - 1, 3)), d)
    codes = np.arange(4 ** k, dtype=np.uint64)
    inp = pagctl.LoadedInput(d, threads=2, outer_sample=outer)
    try:
        ora = pagctl.run_oracle(inp, streams=True, solid_codes=codes)
        assert ora["n_solid"] == 4 ** k
        if how == "codes":
            hip = pagctl.run_hip(inp, streams=True, solid_codes=codes)
        else:
            hip = pagctl.run_hip(inp, streams=True, solid_bitmap=np.full(4 ** k // 32, 0xFFFFFFFF, np.uint32))
        assert hip["n_solid"] == 4 ** k
        pagctl.compare_results(hip, ora, label=f"all solid ({how}) outer={outer}")
        assert hip["stats"].n_pos > 0
        hip_host = pagctl.run_hip(inp, streams=True, prepare=False, solid_codes=codes if how == "codes" else None,
                                  solid_bitmap=None if how == "codes" else np.full(4 ** k // 32, 0xFFFFFFFF, np.uint32))
        pagctl.compare_results(hip_host, ora, label=f"all solid ({how}, host-prepared) outer={outer}")
    finally:
        inp.close()


@pytest.mark.gpu
def test_extract_rejects_outer_sample_out_of_range(inputs):
    """outer_sample 0 and 8: pag_process returns PAG_EINVAL with a message; the handle then still builds what the oracle does."""
    inp = inputs["sparse"]
    lib = pagctl.hip_lib()
    pagctl.keep_streams(True)
    g = pagctl.hip_create(inp)
    try:
        for bad in (0, 8):
            inp.set_outer_sample(bad)
            st = pagctl.BuildStats()
            assert lib.pag_process(g, inp.view, C.byref(st)) == PAG_EINVAL
            assert "outer_sample" in lib.pag_last_error().decode()
            prepared = pagctl._prepared_view(lib, g, inp)
            assert lib.pag_process(g, C.byref(prepared), C.byref(st)) == PAG_EINVAL
        ora = oracle(inp, "sparse", 5)
        inp.set_outer_sample(5)
        hip = pagctl._run(lib, "pag", g, inp, True, pagctl._prepared_view(lib, g, inp))
        pagctl.compare_results(hip, ora, label="after rejected values, outer=5")
    finally:
        lib.pag_destroy(g)
